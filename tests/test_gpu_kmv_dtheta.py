"""
stpy_kmv_dtheta on the device (csrc/kmvgrad.hip) against the longdouble statement of tests/slq_oracle.py, within its bound
eps [(d + 12) S1 + 2 (n + 8) S0] per derivative column, the stpy_kmv bound on the value column and the dot-product bound on the last one
(tests/test_slq_cpu.py shows a working-precision emulation inside the bound with more than 4x room).  Inputs are rounded to float32 so
that one truth serves both types.  A small cross product: every n in {1, 15, 64, 65, 129, 777}, d in {1, 3, 7, 12, 20} and t in {1, 16, 17, 33}
at least once, all four kinds, every kernel instantiation (d <= 4, <= 8, <= 16, beyond) in both types; cols on a width-8 x; padded leading
dimensions; duplicated points (rho == 0 off the diagonal: the Matern 1/2 guard); and n = 2500, d = 3, t = 5, whose j range is cut.
"""
import numpy as np
import pytest
import torch

from tests import kmv_oracle as KO
from tests import slq_oracle as SO

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
TORCH = {"float64": torch.float64, "float32": torch.float32}
# (kind, n, d, t, cols on a width-8 x, duplicated points)
CASES = [
	("se", 1, 1, 1, None, False),
	("matern12", 15, 3, 16, None, True),
	("matern32", 64, 7, 17, None, False),
	("matern52", 65, 12, 33, None, False),
	("se", 129, 20, 33, None, True),
	("matern12", 777, 3, 17, None, False),
	("matern32", 129, 5, 1, KO.WIDE_COLS, False),
	("matern52", 129, 20, 16, None, False),
	("matern12", 64, 12, 1, None, True),
	("se", 2500, 3, 5, None, False),
]
IDS = ["%s-n%d-d%d-t%d%s%s" % (c[0], c[1], c[2], c[3], "-cols" if c[4] else "", "-dup" if c[5] else "") for c in CASES]
KAPPA = 1.3
_TRUTH = {}


def inputs(ci):
	kind, n, d, t, cols, dup = CASES[ci]
	rng = np.random.RandomState(9100 + ci)
	x = rng.uniform(-1, 1, size=(n, 8 if cols else d))
	if dup and n >= 4:
		x[n // 2:n // 2 + n // 4] = x[:n // 4]
	il = rng.uniform(0.5, 3.0, size=(d,)) / np.sqrt(d)
	U, V = rng.standard_normal((t, n)), rng.standard_normal((t, n))
	return tuple(v.astype(np.float32).astype(np.float64) for v in (x, il, U, V))


def truth(ci):
	"""(out, S0, S1, SK, SD) of a case in longdouble, computed once."""
	if ci not in _TRUTH:
		kind, n, d, t, cols, dup = CASES[ci]
		x, il, U, V = inputs(ci)
		_TRUTH[ci] = SO.kmv_dtheta_dense(kind, x, il, U, V, cols=cols, kappa=KAPPA)
	return _TRUTH[ci]


def device(ci, dtype_name, pad=(0, 0, 0), want_y=False):
	from stpy_amd import _lib
	kind, n, d, t, cols, dup = CASES[ci]
	dev, dt = _lib.device(), TORCH[dtype_name]
	x, il, U, V = (torch.from_numpy(v).to(dev, dt) for v in inputs(ci))
	colt = torch.tensor(cols, dtype=torch.int32, device=dev) if cols else None
	Ut = torch.full((t, n + pad[0]), float("nan"), dtype=dt, device=dev)[:, :n]
	Vt = torch.full((t, n + pad[1]), float("nan"), dtype=dt, device=dev)[:, :n]
	Ut.copy_(U)
	Vt.copy_(V)
	out = torch.full((t, d + 2 + pad[2]), float("nan"), dtype=dt, device=dev)[:, :d + 2]
	_lib.kmv_dtheta(KO.KIND_CODE[kind], x, il, Ut, Vt, out, cols=colt, kappa=KAPPA)
	if want_y:
		Y = torch.empty((t, n), dtype=dt, device=dev)
		_lib.kmv(KO.KIND_CODE[kind], x, x, Vt, Y, il, cols=colt, kappa=KAPPA)
		torch.cuda.synchronize()
		return out.cpu().numpy(), Y.cpu().numpy()
	torch.cuda.synchronize()
	return out.cpu().numpy()


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_kmv_dtheta_against_the_longdouble_oracle(ci, dtype_name):
	kind, n, d, t, cols, dup = CASES[ci]
	want, S0, S1, SK, SD = truth(ci)
	bound = SO.kmv_dtheta_bound(n, d, KO.eps_of(TORCH_NP[dtype_name]), S0, S1, SK, SD)
	got = device(ci, dtype_name)
	assert got.shape == (t, d + 2) and np.all(np.isfinite(got))
	err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
	with np.errstate(divide="ignore", invalid="ignore"):
		ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
	print("%s %s: largest error / bound: derivative columns %.4f, value %.4f, dot %.4f" % (
		IDS[ci], dtype_name, ratio[:, :d].max(), ratio[:, d].max(), ratio[:, d + 1].max()))
	assert np.all(err <= bound), (IDS[ci], float(ratio.max()))
	if n == 1:
		assert np.all(got[:, :d] == 0)                                    # the only pair is (i, i): rho == 0 contributes exactly 0


TORCH_NP = {"float64": np.float64, "float32": np.float32}


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("ci", [2, 4, 5, 9], ids=[IDS[i] for i in (2, 4, 5, 9)])
def test_kmv_dtheta_same_bits_twice_and_for_padded_leading_dimensions(ci, dtype_name):
	a = device(ci, dtype_name)
	b = device(ci, dtype_name)
	c = device(ci, dtype_name, pad=(5, 11, 3))
	assert np.array_equal(a, b)
	assert np.array_equal(a, c)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("ci", [3, 6, 9], ids=[IDS[i] for i in (3, 6, 9)])
def test_kmv_dtheta_value_column_is_stpy_kmv_followed_by_a_dot_product(ci, dtype_name):
	"""out[:, d] against <u_c, (K v_c)> with K v_c from stpy_kmv (the dot product in float64 on the host): within the sum of both bounds."""
	kind, n, d, t, cols, dup = CASES[ci]
	_, _, _, SK, _ = truth(ci)
	got, Y = device(ci, dtype_name, want_y=True)
	U = inputs(ci)[2]
	ref = np.sum(U * Y.astype(np.float64), axis=1)
	bound = 2 * (2 * KO.eps_of(TORCH_NP[dtype_name]) * (n + d + 8) * SK)
	assert np.all(np.abs(got[:, d].astype(np.float64) - ref) <= bound)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_kmv_dtheta_duplicated_points_matern12(dtype_name):
	"""Every point twice: half of the off-diagonal pairs have rho == 0, where Matern 1/2's chi is -exp(-r) / r.  Finite, and equal to the
	oracle (whose sum leaves those pairs out) within the bound."""
	from stpy_amd import _lib
	dev, dt = _lib.device(), TORCH[dtype_name]
	rng = np.random.RandomState(77)
	half = rng.uniform(-1, 1, size=(40, 2)).astype(np.float32).astype(np.float64)
	x = np.concatenate([half, half])
	il = np.array([1.5, 0.75])
	U, V = (rng.standard_normal((3, 80)).astype(np.float32).astype(np.float64) for _ in range(2))
	out = torch.empty((3, 4), dtype=dt, device=dev)
	_lib.kmv_dtheta(KO.KIND_CODE["matern12"], torch.from_numpy(x).to(dev, dt), torch.from_numpy(il).to(dev, dt), torch.from_numpy(U).to(dev, dt),
					torch.from_numpy(V).to(dev, dt), out)
	got = out.cpu().numpy()
	want, S0, S1, SK, SD = SO.kmv_dtheta_dense("matern12", x, il, U, V)
	assert np.all(np.isfinite(got))
	assert np.all(np.abs(got.astype(np.longdouble) - want).astype(np.float64) <= SO.kmv_dtheta_bound(80, 2, KO.eps_of(TORCH_NP[dtype_name]), S0, S1, SK, SD))


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_kmv_dtheta_empty_problem_writes_zeros(dtype_name):
	from stpy_amd import _lib
	dev, dt = _lib.device(), TORCH[dtype_name]
	out = torch.full((3, 6), float("nan"), dtype=dt, device=dev)
	x = torch.empty((0, 4), dtype=dt, device=dev)
	_lib.kmv_dtheta(0, x, torch.ones(4, dtype=dt, device=dev), torch.empty((3, 0), dtype=dt, device=dev), torch.empty((3, 0), dtype=dt, device=dev), out)
	assert np.all(out.cpu().numpy() == 0)
