"""
Input gradients of the local experts on the device: stpy_experts_predict_grad / stpy_experts_combine_grad against the NumPy oracle
(tests/experts_grad_oracle.py, itself held to central differences and to an extended-precision restatement by tests/test_experts_grad_cpu.py),
the promises of the header as properties -- mu_e and var_e carry the bits of stpy_experts_predict, mu and var those of stpy_experts_combine; an
expert's four outputs do not depend on the batch around it or on nmax; a failed or mis-sized expert yields the flat prior and leaves its
neighbours alone; nothing is written beside the views -- and LocalExpertsGaussianProcess.mean_std_grad / ucb_optimize against the oracle, the
dense class and themselves.

Tolerance 1e-8 relative to the largest entry of the compared array, as in the rest of the C-ABI suite; 1e-12 entry by entry for the combination
on synthetic inputs.  The fits, cases and helpers are those of tests/test_gpu_experts.py (one border fit per kind serves both files).
"""
import numpy as np
import pytest
import torch

from tests import experts_grad_oracle as GO
from tests import experts_oracle as XO
from tests.test_gpu_experts import CLASS, _border, _class_case, _dev, _fit, _predict

pytestmark = pytest.mark.gpu

TOL = 1e-8
MODES = (XO.POE, XO.GPOE, XO.BCM, XO.RBCM)
NAN = float("nan")


@pytest.fixture(scope="module")
def S(gpu_device):
	import stpy_amd
	return stpy_amd


@pytest.fixture(scope="module")
def ref():
	return XO.reference_case()


WORST = {}          # the largest error seen per group of quantities, for the summaries the tests print


def _close(got, want, scale=None, tol=TOL, what="", group=None):
	scale = float(np.max(np.abs(want))) if scale is None else scale
	err = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) / (scale if scale > 0 else 1.0)
	print(what, "error", err)
	if group is not None:
		WORST[group] = max(WORST.get(group, 0.0), err)
	assert err <= tol, (what, err)


def _predict_grad(dev, st, xt, modes=MODES, pad=0):
	"""one stpy_experts_predict_grad call and one stpy_experts_combine_grad call per mode.  xt: a NumPy array or a device tensor (which may be a
	strided view); pad > 0: every output is the leading view of a NaN-filled buffer wider by pad in each dimension but the experts', and the
	padding is checked to be NaN still.  Returns (mu_e, var_e, gmu_e, gvar_e, {mode: (mu, var, dmu, dstd)}) as NumPy arrays"""
	from stpy_amd import _lib as L
	E, M, d = len(st["sizes"]), xt.shape[0], int(st["inv_ls"].numel())
	xt_d = xt if torch.is_tensor(xt) else _dev(xt, dev)
	full = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device=dev)
	mu_f, var_f, gmu_f, gvar_f = full(E, M + pad), full(E, M + pad), full(E, M + pad, d + pad), full(E, M + pad, d + pad)
	mu_e, var_e, gmu_e, gvar_e = mu_f[:, :M], var_f[:, :M], gmu_f[:, :M, :d], gvar_f[:, :M, :d]
	L.experts_predict_grad(st["kind"], st["xs"], st["offsets"], st["nmax"], st["inv_ls"], st["kappa"], st["factor"], st["alpha"], st["info"], xt_d,
						   mu_e, var_e, gmu_e, gvar_e, cols=st["cols"])
	out, views = {}, [(mu_f, mu_e), (var_f, var_e), (gmu_f, gmu_e), (gvar_f, gvar_e)]
	for mode in modes:
		mu_b, var_b, dmu_b, dstd_b = full(M + pad), full(M + pad), full(M + pad, d + pad), full(M + pad, d + pad)
		mu, var, dmu, dstd = mu_b[:M], var_b[:M], dmu_b[:M, :d], dstd_b[:M, :d]
		L.experts_combine_grad(mode, mu_e, var_e, gmu_e, gvar_e, st["kappa"], mu, var, dmu, dstd)
		out[mode] = tuple(t.cpu().numpy() for t in (mu, var, dmu, dstd))
		views += [(mu_b, mu), (var_b, var), (dmu_b, dmu), (dstd_b, dstd)]
	torch.cuda.synchronize()
	res = (mu_e.cpu().numpy(), var_e.cpu().numpy(), gmu_e.cpu().numpy(), gvar_e.cpu().numpy(), out)
	for buf, view in views:          # nothing beside the views: what is left once the view itself is overwritten is NaN still
		view.zero_()
		assert int(torch.isnan(buf).sum()) == buf.numel() - view.numel()
	return res


def _check_against_oracle(dev, st, orc, g_orc, xt, kappa, what, pad=0, combined=True):
	"""the four per-expert outputs and the combined ones at the test points xt (the oracle's arrays cover them from their start): gradients against
	the oracle, mu_e / var_e bit for bit against stpy_experts_predict, mu / var bit for bit against stpy_experts_combine"""
	M = xt.shape[0]
	gmu_o, gvar_o = g_orc[0][:, :M], g_orc[1][:, :M]
	mu_e, var_e, gmu_e, gvar_e, comb = _predict_grad(dev, st, xt, pad=pad)
	mu_p, var_p, comb_p = _predict(dev, st, xt)
	assert np.array_equal(mu_e, mu_p) and np.array_equal(var_e, var_p), what
	_close(gmu_e, gmu_o, scale=float(np.max(np.abs(g_orc[0]))), what=what + " gmu_e", group="gmu_e")
	_close(gvar_e, gvar_o, scale=float(np.max(np.abs(g_orc[1]))), what=what + " gvar_e", group="gvar_e")
	assert np.all(np.isfinite(gmu_e)) and np.all(np.isfinite(gvar_e))
	for mode in MODES:
		mu, var, dmu, dstd = comb[mode]
		assert np.array_equal(mu, comb_p[mode][0]) and np.array_equal(var, comb_p[mode][1]), (what, mode)
		if combined:
			_, _, dmu_o, dstd_o = GO.combine_grad(mode, orc["mu_e"][:, :M], orc["var_e"][:, :M], gmu_o, gvar_o, kappa)
			_close(dmu, dmu_o, what="%s mode %d dmu" % (what, mode), group="dmu")
			_close(dstd, dstd_o, what="%s mode %d dstd" % (what, mode), group="dstd")
	return mu_e, var_e, gmu_e, gvar_e, comb


# --------------------------------------------------------------------------------------------- per expert, against the oracle
@pytest.mark.parametrize("kind", ["se", "matern12", "matern32", "matern52", "ard"])
def test_reference_case_against_oracle(S, gpu_device, ref, kind):
	"""N = 167, five experts of at most 34, d = 3, 65 test points of which 20 are training points (Matern 1/2: the zero convention); ARD picks its
	coordinates out of wider rows by cols, a lengthscale each"""
	ard = kind == "ard"
	k = XO.SE if ard else {"se": 0, "matern12": 1, "matern32": 2, "matern52": 3}[kind]
	if ard:
		cols, inv_ls = [3, 0, 2], 1.0 / np.array([0.4, 0.7, 0.3])
		widen = lambda x: np.concatenate([x[:, 1:2], 7.0 + x[:, :1], x[:, 2:3], x[:, :1], -x[:, :1]], axis=1)
	else:
		cols, inv_ls, widen = None, ref["inv_ls"], (lambda x: x)
	xs, xt, kappa = widen(ref["xs"]), widen(ref["xt"]), ref["kappa"]
	st = _fit(gpu_device, k, xs, ref["ys"], ref["sizes"], inv_ls, ref["s"], kappa, cols=cols)
	orc = XO.experts(k, xs, ref["ys"], ref["sizes"], inv_ls, ref["s"], kappa, cols=cols, xt=xt)
	assert XO.n_clamped(orc["var_e"], kappa) == 0
	g_orc = GO.experts_grad(k, xs, orc, inv_ls, kappa, xt, cols)
	WORST.clear()
	full = _check_against_oracle(gpu_device, st, orc, g_orc, xt, kappa, kind + " reference M=65")
	part = _check_against_oracle(gpu_device, st, orc, g_orc, xt[:33], kappa, kind + " reference M=33")
	assert all(np.array_equal(a[:, :33], b) for a, b in zip(full[:4], part[:4]))          # a test point's bits do not depend on the tile it sits in
	print("worst gradient errors, %s reference:" % kind, dict(WORST))


# --------------------------------------------------------------------------------------------- every block size up to the cap, in one batch
_BORDER_GRAD = {}


def _border_grad(dev, kind):
	"""the border case of tests/test_gpu_experts.py (its oracle and its device fit, shared with that file) and the oracle's gradients: once per kind"""
	c, orc, st = _border(dev, kind)
	if kind not in _BORDER_GRAD:
		_BORDER_GRAD[kind] = GO.experts_grad(kind, c["xs"], orc, c["inv_ls"], c["kappa"], c["xt"])
	return c, orc, st, _BORDER_GRAD[kind]


@pytest.mark.parametrize("kind", XO.KINDS)
def test_border_against_oracle(S, gpu_device, kind):
	"""experts of 1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 200, 511 and 512 points under nmax = 512 -- where the second triangular product changes
	its round structure -- at M = 97, 33, 32 and 1, where the last tile is ragged, full or a single point"""
	c, orc, st, g_orc = _border_grad(gpu_device, kind)
	assert XO.n_clamped(orc["var_e"], c["kappa"]) == 0
	WORST.clear()
	full = None
	for M in (97, 33, 32, 1):
		got = _check_against_oracle(gpu_device, st, orc, g_orc, c["xt"][:M], c["kappa"], "kind %d border M=%d" % (kind, M))
		if full is None:
			full = got
		else:          # a test point's bits do not depend on M
			assert all(np.array_equal(a[:, :M], b) for a, b in zip(full[:4], got[:4]))
			assert all(np.array_equal(full[4][mode][i][:M], got[4][mode][i]) for mode in MODES for i in range(4))
	print("worst gradient errors, kind %d border:" % kind, dict(WORST))
	# the last test point is 40 units from the data along every axis: flat for every expert
	assert np.all(np.abs(full[2][:, -1]) < 1e-30) and np.all(np.abs(full[3][:, -1]) < 1e-30)


def test_border_layout_variant(S, gpu_device):
	"""xs and xt as rows of width 8 of which cols picks (and permutes) five, NaN in the others; xt a row- and column-sliced view of a wider buffer
	(ldt = 11); every output a view of a wider NaN-filled buffer: the bits of the dense layout, and nothing written beside the views"""
	kind = XO.MATERN52
	c, orc, st, g_orc = _border_grad(gpu_device, kind)
	d, cols = XO.BORDER["d"], [6, 1, 4, 0, 3]

	def wide(a):
		out = np.full((a.shape[0], 8), np.nan)
		out[:, cols] = a
		return out
	stw = _fit(gpu_device, kind, wide(c["xs"]), c["ys"], c["sizes"], c["inv_ls"], c["s"], c["kappa"], cols=cols)
	for M in (97, 33):
		buf = torch.full((M + 3, 11), NAN, dtype=torch.float64, device=gpu_device)
		xt = buf[2:2 + M, 1:9]
		xt.copy_(_dev(wide(c["xt"][:M]), gpu_device))
		assert xt.stride(0) == 11
		w = _check_against_oracle(gpu_device, stw, orc, g_orc, xt, c["kappa"], "wide layout M=%d" % M, pad=5)
		dense = _predict_grad(gpu_device, st, c["xt"][:M])
		assert all(np.array_equal(a, b) and not np.isnan(a).any() for a, b in zip(w[:4], dense[:4]))
		assert all(np.array_equal(w[4][mode][i], dense[4][mode][i]) for mode in MODES for i in range(4))


# --------------------------------------------------------------------------------------------- the header's promises
def test_position_slice_and_batch_independence(S, gpu_device):
	"""an expert's four outputs carry the same bits wherever it sits in whatever batch, whatever nmax sizes the slices, and in a repeated call; the
	last of 300 experts (600 workgroups, more than the CUs of the device) is the expert alone"""
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
		one = _predict_grad(gpu_device, st, xt, modes=())[:4]
		two = _predict_grad(gpu_device, st, xt, modes=())[:4]
		assert all(np.array_equal(a, b) and np.all(np.isfinite(a)) for a, b in zip(one, two))
		return {k: tuple(a[i] for a in one) for i, k in enumerate(names)}

	abc, ca, adc = run("ABC", 128), run("CA", 128), run("ADC", 512)
	for k in "AC":
		for other in (ca, adc):
			for a, b in zip(abc[k], other[k]):
				assert np.array_equal(a, b), k
	# ... and they are the right ones
	for k in "ACD":
		f = XO.expert_fit(kind, blocks[k][0], blocks[k][1], inv_ls, 0.2, 1.1)
		gmu, gvar = GO.expert_grad(kind, blocks[k][0], f, inv_ls, 1.1, xt)
		_close(adc[k][2], gmu, what="block %s gmu" % k)
		_close(adc[k][3], gvar, what="block %s gvar" % k)
	# the last of 300
	E, n, d3, M = 300, 33, 3, 33
	rng = np.random.RandomState(19)
	xs, ys = rng.uniform(0, 1, size=(E * n, d3)), rng.normal(size=E * n)
	xt3 = np.concatenate([xs[[(E - 1) * n, E * n - 1, 0]], rng.uniform(0, 1, size=(M - 3, d3))])
	il3 = np.full(d3, 2.5)
	st = _fit(gpu_device, XO.SE, xs, ys, [n] * E, il3, 0.1, 1.3)
	alone = _fit(gpu_device, XO.SE, xs[(E - 1) * n:], ys[(E - 1) * n:], [n], il3, 0.1, 1.3)
	many, single = _predict_grad(gpu_device, st, xt3, modes=())[:4], _predict_grad(gpu_device, alone, xt3, modes=())[:4]
	assert all(np.array_equal(a[E - 1], b[0]) for a, b in zip(many, single))
	for e in (0, 150, E - 1):
		x, y = xs[e * n:(e + 1) * n], ys[e * n:(e + 1) * n]
		gmu, gvar = GO.expert_grad(XO.SE, x, XO.expert_fit(XO.SE, x, y, il3, 0.1, 1.3), il3, 1.3, xt3)
		_close(many[2][e], gmu, what="expert %d of 300 gmu" % e)
		_close(many[3][e], gvar, what="expert %d of 300 gvar" % e)


@pytest.mark.parametrize("kind", XO.KINDS)
def test_coincident_points(S, gpu_device, ref, kind):
	"""every test point IS a training point (eight of every expert, and one of them twice): finite, and the oracle's values -- for Matern 1/2 with
	the coincident pair left out of the sums, the convention of stpy_gram_grad"""
	off = np.concatenate([[0], np.cumsum(ref["sizes"])])
	pick = np.concatenate([off[e] + np.arange(8) * 4 for e in range(len(ref["sizes"]))] + [[0]])
	xt, kappa = ref["xs"][pick], ref["kappa"]
	st = _fit(gpu_device, kind, ref["xs"], ref["ys"], ref["sizes"], ref["inv_ls"], ref["s"], kappa)
	orc = XO.experts(kind, ref["xs"], ref["ys"], ref["sizes"], ref["inv_ls"], ref["s"], kappa, xt=xt)
	assert XO.n_clamped(orc["var_e"], kappa) == 0
	g_orc = GO.experts_grad(kind, ref["xs"], orc, ref["inv_ls"], kappa, xt)
	assert np.all(np.isfinite(g_orc[0])) and np.all(np.isfinite(g_orc[1]))
	_check_against_oracle(gpu_device, st, orc, g_orc, xt, kappa, "kind %d coincident" % kind)


def test_failed_and_missized_experts(S, gpu_device, ref):
	"""an expert whose fit failed (the non-positive-definite construction of test_failing_expert) and one with more rows than nmax (info = -1):
	mu_e = 0, var_e = kappa, zero gradients; the neighbours carry the bits they have in a batch without the offender"""
	sizes = [40, 20, 33]
	rng = np.random.RandomState(2)
	xs = rng.uniform(0, 1, size=(sum(sizes), 3))
	ys = rng.normal(size=sum(sizes))
	xs[40 + 1] = xs[40 + 0]          # expert 1: two coincident points, no noise, kappa = 1: its second pivot is fma(-1, 1, 1) = 0 exactly
	bad = _fit(gpu_device, XO.SE, xs, ys, sizes, ref["inv_ls"], 0.0, 1.0)
	keep = np.r_[0:40, 60:93]
	good = _fit(gpu_device, XO.SE, xs[keep], ys[keep], [40, 33], ref["inv_ls"], 0.0, 1.0, nmax=40)
	assert bad["info_h"].tolist() == [0, 2, 0] and not good["info_h"].any()
	xt = rng.uniform(0, 1, size=(37, 3))
	b, g = _predict_grad(gpu_device, bad, xt), _predict_grad(gpu_device, good, xt)
	assert np.all(b[0][1] == 0.0) and np.all(b[1][1] == 1.0) and np.all(b[2][1] == 0.0) and np.all(b[3][1] == 0.0)
	assert all(np.array_equal(x[[0, 2]], y) for x, y in zip(b[:4], g[:4]))
	# the flat prior of the failed expert counts in the combination as it does in stpy_experts_combine; its gradient is zero
	for mode in MODES:
		_, _, dmu_o, dstd_o = GO.combine_grad(mode, b[0], b[1], b[2], b[3], 1.0)
		assert np.allclose(b[4][mode][2], dmu_o, rtol=1e-12, atol=1e-12 * np.max(np.abs(dmu_o)))
		assert np.allclose(b[4][mode][3], dstd_o, rtol=1e-12, atol=1e-12 * np.max(np.abs(dstd_o)))
	# a middle expert of 40 rows under nmax = 32
	sizes = [20, 40, 32, 5]
	xs, ys = rng.uniform(0, 1, size=(sum(sizes), 3)), rng.normal(size=sum(sizes))
	keep = np.r_[0:20, 60:sum(sizes)]
	bad = _fit(gpu_device, XO.SE, xs, ys, sizes, ref["inv_ls"], 0.1, 1.3, nmax=32)
	good = _fit(gpu_device, XO.SE, xs[keep], ys[keep], [20, 32, 5], ref["inv_ls"], 0.1, 1.3, nmax=32)
	assert bad["info_h"].tolist() == [0, -1, 0, 0] and not good["info_h"].any()
	b, g = _predict_grad(gpu_device, bad, xt, modes=()), _predict_grad(gpu_device, good, xt, modes=())
	assert np.all(b[0][1] == 0.0) and np.all(b[1][1] == 1.3) and np.all(b[2][1] == 0.0) and np.all(b[3][1] == 0.0)
	assert all(np.array_equal(x[[0, 2, 3]], y) for x, y in zip(b[:4], g[:4]))


# --------------------------------------------------------------------------------------------- the combination alone
def test_combine_grad_on_synthetic_inputs(S, gpu_device):
	"""E = 5, M = 50, d = 3, hand-made: expert variances below kappa 2^-52, zero, negative, equal to kappa and above it, one expert at a time and
	all at once, random gradient arrays.  dmu and dstd within 1e-12 of the oracle ENTRY BY ENTRY (exact zeros where every expert is clamped),
	mu and var the bits of stpy_experts_combine"""
	from stpy_amd import _lib as L
	c = GO.synthetic_combine_case()
	S_, kappa = GO.SYNTH, GO.SYNTH["kappa"]
	dev = gpu_device
	mu_e, var_e, gmu_e, gvar_e = (_dev(c[k], dev) for k in ("mu_e", "var_e", "gmu_e", "gvar_e"))
	full = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device=dev)
	for mode in MODES:
		mu, var, dmu, dstd, mu0, var0 = full(S_["M"]), full(S_["M"]), full(S_["M"], S_["d"]), full(S_["M"], S_["d"]), full(S_["M"]), full(S_["M"])
		L.experts_combine_grad(mode, mu_e, var_e, gmu_e, gvar_e, kappa, mu, var, dmu, dstd)
		L.experts_combine(mode, mu_e, var_e, kappa, mu0, var0)
		assert torch.equal(mu, mu0) and torch.equal(var, var0), mode
		mu_o, var_o, dmu_o, dstd_o = GO.combine_grad(mode, c["mu_e"], c["var_e"], c["gmu_e"], c["gvar_e"], kappa)
		for name, got, want in (("mu", mu, mu_o), ("var", var, var_o), ("dmu", dmu, dmu_o), ("dstd", dstd, dstd_o)):
			got = got.cpu().numpy()
			nz = want != 0
			print("mode", mode, name, "worst entrywise error", float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))), "exact zeros", int((~nz).sum()))
			assert np.all(np.isfinite(got)) and np.allclose(got, want, rtol=1e-12, atol=0), (mode, name)


def test_refusals_through_the_wrappers(S, gpu_device, ref):
	"""the documented codes, raised before any launch: a short workspace (-20), a null array (-3), bad gradient strides (-19), a bad mode (-10)"""
	from stpy_amd import _lib as L
	st = _fit(gpu_device, XO.SE, ref["xs"], ref["ys"], ref["sizes"], ref["inv_ls"], ref["s"], ref["kappa"])
	E, M, d = 5, 40, 3
	xt = _dev(ref["xt"][:M], gpu_device)
	z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=gpu_device)
	mu_e, var_e, gmu_e, gvar_e = z(E, M), z(E, M), z(E, M, d), z(E, M, d)
	args = (st["kind"], st["xs"], st["offsets"], st["nmax"], st["inv_ls"], st["kappa"], st["factor"], st["alpha"], st["info"], xt)
	lib = L.load()
	need = lib.stpy_experts_predict_grad_workspace_bytes(0, st["nmax"], d, E, M)
	assert need == 2 * lib.stpy_experts_predict_workspace_bytes(0, st["nmax"], d, E, M) == 2 * 5 * 2 * 32 * 64 * 8
	with pytest.raises(L.StpyHipError, match=r"rc=-20"):
		L.experts_predict_grad(*args, mu_e, var_e, gmu_e, gvar_e, work=torch.empty(need - 16, dtype=torch.uint8, device=gpu_device))
	with pytest.raises(L.StpyHipError, match=r"rc=-3"):
		L.experts_predict_grad(*args[:7], None, *args[8:], mu_e, var_e, gmu_e, gvar_e)
	with pytest.raises(L.StpyHipError, match=r"rc=-19"):          # rows of the gradient arrays that overlap: ldg = 2 < d
		L.experts_predict_grad(*args, mu_e, var_e, gmu_e.as_strided((E, M, d), (M * d, 2, 1)), gvar_e.as_strided((E, M, d), (M * d, 2, 1)))
	with pytest.raises(L.StpyHipError, match=r"rc=-10"):
		L.experts_combine_grad(4, mu_e, var_e, gmu_e, gvar_e, st["kappa"], z(M), z(M), z(M, d), z(M, d))
	with pytest.raises(L.StpyHipError, match=r"rc=-19"):
		L.experts_combine_grad(3, mu_e, var_e, gmu_e, gvar_e, st["kappa"], z(M), z(M), z(M * d).as_strided((M, d), (2, 1)), z(M * d).as_strided((M, d), (2, 1)))
	torch.cuda.synchronize()
	assert not mu_e.any() and not gmu_e.any()          # nothing was launched


# --------------------------------------------------------------------------------------------- the class against the oracle
def _class_oracle(order, sizes, xt, cols=None, inv_ls=None, x=None):
	c, C = _class_case(), CLASS
	x = c["x"] if x is None else x
	inv_ls = np.full(C["d"], 1.0 / C["ls"]) if inv_ls is None else inv_ls
	orc = XO.experts(XO.SE, x[order], c["y"][order], sizes, inv_ls, C["s"], C["kappa"], cols=cols, xt=xt)
	assert XO.n_clamped(orc["var_e"], C["kappa"]) == 0
	return orc, GO.experts_grad(XO.SE, x[order], orc, inv_ls, C["kappa"], xt, cols)


def test_class_mean_std_grad_against_oracle(S, gpu_device):
	"""N = 700 under the explicit partition 512 / 0 / 97 / 1 / 90: the four combinations against the oracle, the chunked path (three chunks) bit
	for bit, expert_mean_var_grad, the launch count"""
	c, C = _class_case(), CLASS
	le = S.LocalExpertsGaussianProcess(gamma=C["ls"], s=C["s"], kappa=C["kappa"], d=C["d"], expert_size=C["expert_size"], partition=torch.from_numpy(c["ids"]))
	le.fit_gp(torch.from_numpy(c["x"]), torch.from_numpy(c["y"]).reshape(-1, 1))
	order, sizes = XO.partition(C["N"], C["expert_size"], c["ids"], 0)
	assert sizes == C["id_sizes"]
	orc, (gmu_o, gvar_o) = _class_oracle(order, sizes, c["xt"])
	xt = torch.from_numpy(c["xt"])
	for name, mode in (("poe", XO.POE), ("gpoe", XO.GPOE), ("bcm", XO.BCM), ("rbcm", XO.RBCM)):
		le.combine, le.max_size = name, 10000
		before = le.launches
		dmu, dstd = le.mean_std_grad(xt)
		assert le.launches - before == 2 and tuple(dmu.shape) == tuple(dstd.shape) == (C["M"], C["d"]) and not dmu.is_cuda
		_, _, dmu_o, dstd_o = GO.combine_grad(mode, orc["mu_e"], orc["var_e"], gmu_o, gvar_o, C["kappa"])
		_close(dmu.numpy(), dmu_o, what="class %s dmu" % name)
		_close(dstd.numpy(), dstd_o, what="class %s dstd" % name)
		le.max_size = 17          # three chunks: the bits of one
		before = le.launches
		dmu_c, dstd_c = le.mean_std_grad(xt)
		assert le.launches - before == 6 and torch.equal(dmu, dmu_c) and torch.equal(dstd, dstd_c)
	le.max_size = 10000
	mu_e, var_e, gmu_e, gvar_e = le.expert_mean_var_grad(xt)
	mu_p, var_p = le.expert_mean_var(xt)
	assert torch.equal(mu_e, mu_p) and torch.equal(var_e, var_p) and tuple(gmu_e.shape) == tuple(gvar_e.shape) == (5, C["M"], C["d"])
	_close(gmu_e.numpy(), gmu_o, what="class gmu_e")
	_close(gvar_e.numpy(), gvar_o, what="class gvar_e")
	le.max_size = 17
	chunked = le.expert_mean_var_grad(xt)
	assert all(torch.equal(a, b) for a, b in zip((mu_e, var_e, gmu_e, gvar_e), chunked))
	# a device tensor in, device tensors out; the refusal of autograd through the test tensor stays and names the way
	dmu_d, dstd_d = le.mean_std_grad(xt.to(gpu_device))
	assert dmu_d.is_cuda and torch.equal(dmu_d.cpu(), le.mean_std_grad(xt)[0])
	with pytest.raises(NotImplementedError, match="mean_std_grad"):
		le.mean_std(xt.clone().requires_grad_(True))


def test_class_ard_on_a_column_group(S, gpu_device):
	"""an ARD kernel on three of five columns (the other two NaN), in an order of its own: the gradients land in the columns the term reads, in
	the term's order, and the other columns are zero"""
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
	orc, (gmu_o, gvar_o) = _class_oracle(order, sizes, c["xt"], inv_ls=1.0 / ag[group])
	dmu, dstd = le.mean_std_grad(torch.from_numpy(wide(c["xt"])))
	assert tuple(dmu.shape) == tuple(dstd.shape) == (C["M"], 5)
	assert torch.all(dmu[:, [1, 4]] == 0) and torch.all(dstd[:, [1, 4]] == 0)
	_, _, dmu_o, dstd_o = GO.combine_grad(XO.RBCM, orc["mu_e"], orc["var_e"], gmu_o, gvar_o, C["kappa"])
	_close(dmu.numpy()[:, group], dmu_o, what="ard group dmu")
	_close(dstd.numpy()[:, group], dstd_o, what="ard group dstd")


def test_one_expert_is_the_dense_gp(S, gpu_device):
	"""one expert under PoE is the exact GP: mean_std_grad against GaussianProcess.mean_std_grad within 1e-7, the tolerance of
	test_one_expert_is_the_dense_gp for gradients; and the acquisition of the dense class at the point ucb_optimize returns"""
	n, d, s, kappa, ls = 200, 3, 0.15, 1.3, 0.6
	rng = np.random.RandomState(7)
	x = rng.uniform(-1, 1, size=(n, d))
	y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, 2]) + 0.1 * rng.normal(size=n)
	xT, yT, xtT = torch.from_numpy(x), torch.from_numpy(y).reshape(-1, 1), torch.from_numpy(rng.uniform(-1.2, 1.2, size=(37, d)))
	bounds = [(-1.0, 1.0)] * d
	le = S.LocalExpertsGaussianProcess(gamma=ls, s=s, kappa=kappa, d=d, expert_size=n, combine="poe", bounds=bounds)
	le.fit_gp(xT, yT)
	gp = S.GaussianProcess(gamma=ls, s=s, kappa=kappa, d=d, bounds=bounds)
	gp.fit_gp(xT, yT)
	assert le.experts_info["E"] == 1
	dmu, dstd = le.mean_std_grad(xtT)
	dmu0, dstd0 = gp.mean_std_grad(xtT)
	_close(dmu.numpy(), dmu0.numpy(), tol=1e-7, what="dmu against GaussianProcess")
	_close(dstd.numpy(), dstd0.numpy(), tol=1e-7, what="dstd against GaussianProcess")
	for lcb in (False, True):
		np.random.seed(3)
		sol, val = le.ucb_optimize(4.0, multistart=4, lcb=lcb)
		mu, sd = gp.mean_std(sol.reshape(1, -1))
		acq = float(mu) + (-2.0 if lcb else 2.0) * float(sd)
		print("one expert, lcb", lcb, "solution", sol.numpy(), "value", float(val), "dense acquisition", acq, "evaluations", le.optimize_info["evaluations"])
		assert abs(float(val) - acq) <= 1e-7 * abs(acq)


# --------------------------------------------------------------------------------------------- ucb_optimize
def test_ucb_optimize(S, gpu_device, ref):
	"""the reference case under the bounding box of its data, eight starts: the solution lies in the box, is no worse than any start, carries the
	acquisition mean_std gives there, repeats under the same seed, and lcb flips the sign convention as in the dense class"""
	lo, hi = ref["x"].min(axis=0), ref["x"].max(axis=0)
	bounds = [(float(a), float(b)) for a, b in zip(lo, hi)]
	le = S.LocalExpertsGaussianProcess(gamma=XO.REF["ls"], s=ref["s"], kappa=ref["kappa"], d=XO.REF["d"], expert_size=XO.REF["expert_size"], bounds=bounds)
	with pytest.raises(NotImplementedError):          # not fitted: nothing to climb
		le.ucb_optimize(4.0, multistart=8)
	le.fit_gp(torch.from_numpy(ref["x"]), torch.from_numpy(ref["y"]).reshape(-1, 1))
	assert le.experts_info["sizes"] == ref["sizes"]
	beta, runs = 4.0, {}
	for key, lcb in (("ucb", False), ("again", False), ("lcb", True)):
		np.random.seed(11)
		before = le.launches
		sol, val = le.ucb_optimize(beta, multistart=8, lcb=lcb)
		info = le.optimize_info
		assert tuple(sol.shape) == (3,) and val.dim() == 0
		assert np.all(sol.numpy() >= lo) and np.all(sol.numpy() <= hi)
		assert info["starts"].shape == (8, 3) and info["start_values"].shape == (8,) and np.all(float(val) >= info["start_values"])
		# every evaluation but the last is a gradient evaluation of two launches, the last the two launches of mean_std
		assert info["launches"] == le.launches - before == 2 * info["evaluations"]
		mu, sd = le.mean_std(sol.reshape(1, -1))
		acq = float(mu) + (-1.0 if lcb else 1.0) * np.sqrt(beta) * float(sd)
		print(key, "solution", sol.numpy(), "value", float(val), "acquisition from mean_std", acq, "evaluations", info["evaluations"], "best start", float(info["start_values"].max()))
		assert abs(float(val) - acq) <= 1e-10 * abs(acq)
		runs[key] = (sol, val, info)
	assert torch.equal(runs["ucb"][0], runs["again"][0]) and torch.equal(runs["ucb"][1], runs["again"][1])
	assert np.array_equal(runs["ucb"][2]["starts"], runs["lcb"][2]["starts"])          # the same draws
	# the start values are the acquisition at the starts, under either sign
	for key, sign in (("ucb", 1.0), ("lcb", -1.0)):
		mu, sd = le.mean_std(torch.from_numpy(runs[key][2]["starts"]))
		assert np.allclose(runs[key][2]["start_values"], (mu + sign * 2.0 * sd).numpy().ravel(), rtol=1e-12, atol=0)
	assert float(runs["lcb"][1]) < float(runs["ucb"][1])
	le.bounds = bounds[:2]
	with pytest.raises(ValueError):
		le.ucb_optimize(beta, multistart=8)
	le.bounds = None
	with pytest.raises(ValueError):
		le.ucb_optimize(beta, multistart=8)
