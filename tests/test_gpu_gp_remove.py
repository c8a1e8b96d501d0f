"""
Row deletion on the device: stpy_potrf_delete (csrc/cholupdate.hip) and GaussianProcess.remove_data_point built on it.  The checker
is, on the device, stpy_potrf of the tile-padded K[R,R] + s^2 I (R the kept rows): the factor after a deletion must be that factor in
the same layout, so every consumer runs on it unchanged; and for the estimator a fresh fit on the kept rows.  Data: the recipe of
tests/test_gp_append.py (seed 11, U(0,1)^3, SE gamma = 0.5, s = 0.3).  tests/test_gp_remove_cpu.py states the identity in NumPy; there
the new factor agrees with the refit to 4e-14 (fp64) / 1.2e-7 (fp32) and the posterior to 1.7e-13 / 1.6e-5, which is the margin under
the bounds below (those of test_gp_append.py for the same comparisons).
"""
import numpy as np
import pytest
import torch

from tests.conftest import golden, rel_err
from tests.test_gp_append import X_ALL, Y_ALL, assert_same_posterior, device_factor, pad, se_gram, trsv
from tests.test_gp_remove_cpu import kept

IB = 128
GAMMA, S_NOISE = 0.5, 0.3
_CACHE = {}


def gram(n0):
	if n0 not in _CACHE:
		_CACHE[n0] = se_gram(X_ALL[:n0], gamma=GAMMA, s=S_NOISE)
	return _CACHE[n0]


ABI_CASES = {
	"2-last": (2, [1]),
	"129-one-tile": (129, [5]),                         # one tile: no row kernel
	"257-to-256": (257, [256]),                         # n1 a tile multiple: no border
	"300-first": (300, [0]),
	"300-last": (300, [299]),                           # no rotation
	"385-straddle": (385, [127, 128, 129]),             # straddles a tile, the padded order shrinks 512 -> 384
	"385-ends": (385, [0, 130, 384]),
	"300-scattered": (300, [3, 77, 128, 201, 290]),     # KC = 8
	"1030-every-33rd": (1030, list(range(0, 1030, 33))[:32]),      # k = 32
	"640-k40": (640, list(range(100, 140))),            # two chunks
}


def deleted(n0, S, dtype, fill=7.0):
	"""stpy_potrf_delete through the typed wrapper, into buffers pre-filled with garbage.  Returns (A before, A after, B, winv, info)."""
	from stpy_amd import _lib
	A, _ = device_factor(gram(n0), dtype)
	A0 = A.clone()
	n1p = pad(n0 - len(S))
	B = torch.full((n1p, n1p), fill, dtype=dtype, device="cuda")
	winv = torch.full((_lib.potrf_winv_elems(n1p),), 5.0, dtype=dtype, device="cuda")
	info = _lib.potrf_delete(A, n0, S, B, winv)
	torch.cuda.synchronize()
	_lib.check_async("delete")
	return A0, A, B, winv, int(info.item())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", list(ABI_CASES))
def test_delete_matches_factor_of_kept_rows(gpu_device, case, dtype):
	n0, S = ABI_CASES[case]
	R = kept(n0, S)
	n1 = len(R)
	n1p = pad(n1)
	f64 = dtype == torch.float64
	A0, A, B, w, info = deleted(n0, S, dtype)
	assert info == 0
	assert torch.equal(A, A0)                                                        # the source is not written
	Lf, wf = device_factor(gram(n0)[np.ix_(R, R)], dtype)
	got = torch.tril(B[:n1, :n1]).double().cpu().numpy()
	ref = torch.tril(Lf[:n1, :n1]).double().cpu().numpy()
	err = rel_err(got, ref)
	print("%s %s: factor against stpy_potrf of the kept rows %.2e" % (case, dtype, err))
	assert err < (1e-11 if f64 else 1e-4)
	# the layout stpy_potrf leaves: identity border, zeros above the diagonal of every diagonal tile
	assert torch.equal(B[n1:n1p, :n1p], torch.eye(n1p, dtype=dtype, device="cuda")[n1:n1p])
	for c in range(0, n1p, IB):
		T = B[c:c + IB, c:c + IB]
		assert torch.equal(torch.triu(T, 1), torch.zeros_like(T))
		inv = torch.linalg.inv(torch.tril(T).double())
		blk = w[(c // IB) * IB * IB:(c // IB + 1) * IB * IB].reshape(IB, IB).double()
		assert rel_err(blk.cpu().numpy(), inv.cpu().numpy()) < (1e-12 if f64 else 1e-4)
	# the vector solves run on (B, winv) as on the refit's factor
	y = torch.from_numpy(Y_ALL[:n0].reshape(-1)[R]).to(dtype).cuda()
	for trans in (0, 1):
		a, b = trsv(B, w, n1p, y, trans), trsv(Lf, wf, n1p, y, trans)
		assert rel_err(a.double().cpu().numpy(), b.double().cpu().numpy()) < (1e-11 if f64 else 1e-4)
	# bit-reproducible
	_, _, B2, w2, _ = deleted(n0, S, dtype)
	lower = torch.tril(torch.ones((n1p, n1p), dtype=torch.bool, device="cuda"))
	assert torch.equal(B[lower], B2[lower]) and torch.equal(w, w2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_block_columns_left_of_the_deleted_row_are_copies(gpu_device, dtype):
	"""(1030, [900]): the rotations start at block column 896; everything to its left is bit for bit the old factor"""
	A0, _, B, _, info = deleted(1030, [900], dtype)
	assert info == 0
	assert torch.equal(torch.tril(B[:896, :896]), torch.tril(A0[:896, :896]))
	assert torch.equal(B[896:900, :896], A0[896:900, :896]) and torch.equal(B[900:1029, :896], A0[901:1030, :896])
	assert not torch.equal(B[900:1029, 896:1029], A0[901:1030, 896:1029])          # ... and the rest was rotated


@pytest.mark.gpu
def test_tiles_above_the_diagonal_are_left_alone(gpu_device):
	_, _, B, _, _ = deleted(385, [127, 128, 129], torch.float64, fill=7.0)
	for bi in range(3):
		for bj in range(bi + 1, 3):
			assert bool((B[bi * IB:(bi + 1) * IB, bj * IB:(bj + 1) * IB] == 7.0).all())


@pytest.mark.gpu
def test_unaligned_destination_takes_the_element_stores(gpu_device):
	"""a destination whose rows are not 16-byte aligned (odd leading dimension, offset base): same numbers"""
	from stpy_amd import _lib
	n0, S = 300, [0, 150]
	A, _ = device_factor(gram(n0), torch.float64)
	n1p = pad(n0 - len(S))
	w1 = torch.empty((_lib.potrf_winv_elems(n1p),), dtype=torch.float64, device="cuda")
	w2 = torch.empty_like(w1)
	B1 = torch.zeros((n1p, n1p), dtype=torch.float64, device="cuda")
	wide = torch.zeros((n1p, n1p + 3), dtype=torch.float64, device="cuda")
	B2 = wide[:, 1:n1p + 1]
	i1, i2 = _lib.potrf_delete(A, n0, S, B1, w1), _lib.potrf_delete(A, n0, S, B2, w2)
	assert int(i1.item()) == 0 and int(i2.item()) == 0
	assert torch.equal(torch.tril(B1), torch.tril(B2)) and torch.equal(w1, w2)
	assert bool((wide[:, 0] == 0).all()) and bool((wide[:, n1p + 1:] == 0).all())


# ---------------------------------------------------------------- the estimator
def gp_new(gamma=GAMMA, s=S_NOISE):
	from stpy_amd import GaussianProcess
	return GaussianProcess(gamma=gamma, s=s, kappa=1.0, kernel_name="squared_exponential", d=3)


def xy(n, dtype, lo=0):
	return torch.from_numpy(X_ALL[lo:lo + n]).to(dtype), torch.from_numpy(Y_ALL[lo:lo + n]).to(dtype)


XT = np.random.RandomState(9).uniform(0, 1, size=(50, 3))

GP_CASES = {"300-first": (300, [0]), "300-last": (300, [-1]), "385-straddle": (385, [127, 128, 129]), "385-ends": (385, [0, 130, 384]),
			"640-k40": (640, list(range(100, 140)))}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", list(GP_CASES))
def test_remove_matches_a_fresh_fit(gpu_device, case, dtype):
	n0, S = GP_CASES[case]
	R = kept(n0, [s % n0 for s in S])
	x, y = xy(n0, dtype)
	xt = torch.from_numpy(XT).to(dtype)
	tol = 1e-10 if dtype == torch.float64 else 1e-4
	GPf = gp_new()
	GPf.fit_gp(x[R], y[R])
	GP = gp_new()
	GP.fit_gp(x, y)
	GP.remove_data_point(S if len(S) > 1 else S[0], iterative=True)
	assert GP.remove_path == "update" and GP.n == len(R) and GP.fitted
	assert torch.equal(GP.x, x[R]) and torch.equal(GP.y, y[R])
	assert tuple(GP._L.shape) == (pad(len(R)), pad(len(R))) and GP._Lbuf.shape[0] == pad(n0)          # same capacity as the buffer it replaced
	assert_same_posterior(GP, GPf, xt, tol)
	# the default route: slice and refit
	GP2 = gp_new()
	GP2.fit_gp(x, y)
	GP2.remove_data(torch.tensor(S))
	assert GP2.remove_path == "refit" and GP2.n == len(R)
	assert_same_posterior(GP2, GPf, xt, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_append_after_remove_stays_in_place(gpu_device, dtype):
	x, y = xy(301, dtype)
	xt = torch.from_numpy(XT).to(dtype)
	GP = gp_new()
	GP.fit_gp(x[:300], y[:300])
	GP.remove_data_point([4, 200], iterative=True)
	assert GP.remove_path == "update"
	p, cap = GP._Lbuf.data_ptr(), GP._Lbuf.shape[0]
	GP.add_data_point(x[300:], y[300:], iterative=True)
	assert GP._Lbuf.data_ptr() == p and GP._L.data_ptr() == p and GP._Lbuf.shape[0] == cap and GP.n == 299
	R = kept(301, [4, 200])
	GPf = gp_new()
	GPf.fit_gp(x[R], y[R])
	assert_same_posterior(GP, GPf, xt, 1e-10 if dtype == torch.float64 else 1e-4)


@pytest.mark.gpu
def test_sliding_window(gpu_device):
	"""32 steps of append one / delete the oldest at n = 300, fp64, every step against a refit (fp32 drifts to 3.9e-5 in the NumPy
	statement: too close to 1e-4 to assert)"""
	n, steps = 300, 32
	x, y = xy(n + steps, torch.float64)
	xt = torch.from_numpy(XT)
	GP = gp_new()
	GP.fit_gp(x[:n], y[:n])
	for t in range(steps):
		GP.add_data_point(x[n + t:n + t + 1], y[n + t:n + t + 1], iterative=True)
		GP.remove_data_point(0, iterative=True)
		assert GP.remove_path == "update" and GP.n == n
		GPf = gp_new()
		GPf.fit_gp(x[t + 1:n + t + 1], y[t + 1:n + t + 1])
		assert torch.equal(GP.x, GPf.x)
		assert_same_posterior(GP, GPf, xt, 1e-10)


@pytest.mark.gpu
def test_fallbacks_refit(gpu_device):
	from stpy_amd import GaussianProcess
	n0, S = 300, [0, 150, 299]
	R = kept(n0, S)
	x, y = xy(n0, torch.float64)
	xt = torch.from_numpy(XT)
	# a changed gamma: the factor no longer matches, the call refits under the new gamma
	GP = gp_new(gamma=0.4)
	GP.fit_gp(x, y)
	GP.kernel_object.params_dict['0']['gamma'] = 0.7
	GP.remove_data_point(S, iterative=True)
	assert GP.remove_path == "refit"
	GPf = gp_new(gamma=0.7)
	GPf.fit_gp(x[R], y[R])
	assert_same_posterior(GP, GPf, xt, 1e-10)
	# an explicit diagonal Sigma is kept as Sigma[R][:, R]
	Sig = torch.diag(torch.linspace(0.1, 0.3, n0, dtype=torch.float64))
	GA = gp_new()
	GA.add_data_point(x, y, Sigma=Sig)
	GA.remove_data_point(S, iterative=True)
	assert GA.remove_path == "refit" and torch.equal(GA._Sigma, Sig[R][:, R])
	GB = gp_new()
	GB.fit_gp(x[R], y[R], Sigma=Sig[R][:, R])
	assert_same_posterior(GA, GB, xt, 1e-10)
	# ... any other Sigma is refused, and nothing changes
	GC = gp_new()
	full = Sig.clone()
	full[0, 1] = 0.01
	GC.fit_gp(x, y, Sigma=full)
	F = GC._factor
	with pytest.raises(ValueError):
		GC.remove_data_point(S)
	assert GC.n == n0 and GC._factor is F and GC.fitted
	# more rows than delete_max_rank
	GD = gp_new()
	GD.fit_gp(x, y)
	GD.delete_max_rank = 2
	GD.remove_data_point(S, iterative=True)
	assert GD.remove_path == "refit"
	GE = gp_new()
	GE.fit_gp(x[R], y[R])
	assert_same_posterior(GD, GE, xt, 1e-10)


@pytest.mark.gpu
def test_refused_calls_change_nothing(gpu_device):
	x, y = xy(200, torch.float64)
	GP = gp_new()
	GP.fit_gp(x, y)
	F, x0 = GP._factor, GP.x
	for it in (False, True):
		for bad, exc in (([3, 3], ValueError), ([5, -195], ValueError), (200, IndexError), ([0, -201], IndexError), (list(range(200)), ValueError),
						 (torch.arange(200), ValueError), (1.0, TypeError)):
			with pytest.raises(exc):
				GP.remove_data_point(bad, iterative=it)
			assert GP.x is x0 and GP.n == 200 and GP.fitted is True and GP._factor is F
	GP.remove_data_point([], iterative=True)          # nothing to remove: nothing happens
	assert GP.x is x0 and GP.n == 200 and GP._factor is F


@pytest.mark.gpu
def test_G1_with_three_points_removed(gpu_device):
	"""the reference's semantics (forgetting = fitting on the kept rows): golden G1's data, oracle fitted on the kept rows"""
	from oracle import gp_oracle as O
	from stpy_amd import GaussianProcess
	g = golden("G1_c1_s01")
	n0 = g["x"].shape[0]
	assert n0 == 512
	S = [0, 200, 511]
	R = kept(n0, S)
	GP = GaussianProcess(gamma=float(g["gamma"]), s=float(g["s"]), kappa=float(g["kappa"]), kernel_name="squared_exponential", d=1)
	GP.fit_gp(torch.from_numpy(g["x"]), torch.from_numpy(g["y"]))
	GP.remove_data_point(S, iterative=True)
	assert GP.remove_path == "update"
	mu, std = GP.mean_std(torch.from_numpy(g["xtest"]))
	spec = [("squared_exponential", {"gamma": float(g["gamma"]), "kappa": float(g["kappa"])}, "-")]
	L, alpha = O.fit(g["x"][R], g["y"][R], spec, float(g["s"]))
	mu_o, std_o = O.mean_std(g["x"][R], L, alpha, g["xtest"], spec)
	e_mu, e_std = rel_err(mu.cpu().numpy(), mu_o), rel_err(std.cpu().numpy(), std_o)
	print("G1 minus three points: mu %.2e std %.2e" % (e_mu, e_std))
	assert e_mu < 1e-8 and e_std < 1e-8
