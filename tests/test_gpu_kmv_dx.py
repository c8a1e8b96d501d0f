"""
stpy_kmv_dx on the device (csrc/kmvdx.hip) against the longdouble statement of tests/pathwise_oracle.py, within its bound
eps [(d + 12) S1 + 2 (q + 8) S0] per gradient entry and the stpy_kmv bound on the value column (tests/test_pathwise_cpu.py shows a
working-precision emulation inside the bound).  Inputs are rounded to float32 so that one truth serves both types.  A small cross product:
every n in {1, 15, 64, 65, 129}, q in {1, 63, 65, 777}, d in {1, 3, 7, 12, 20} and t in {1, 16, 17, 33} at least once, all four kinds, every
kernel instantiation (d <= 4, <= 8, <= 16, beyond) in both types; cols on a width-8 x; query points that coincide with contracted points
(rho == 0: the Matern 1/2 guard); a and b of different widths; padded leading dimensions; and n = 5, q = 2500, d = 3, t = 5, whose j range is cut.
"""
import numpy as np
import pytest
import torch

from tests import kmv_oracle as KO
from tests import pathwise_oracle as PO

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
TORCH = {"float64": torch.float64, "float32": torch.float32}
TORCH_NP = {"float64": np.float64, "float32": np.float32}
# (kind, n, q, d, t, cols on a width-8 x, coinciding points, extra columns of b)
CASES = [
	("se", 1, 1, 1, 1, None, False, 0),
	("matern12", 15, 63, 3, 16, None, True, 0),
	("matern32", 64, 65, 7, 17, None, False, 0),
	("matern52", 65, 777, 12, 33, None, False, 0),
	("se", 129, 63, 20, 33, None, True, 0),
	("matern12", 129, 777, 20, 16, None, False, 0),
	("matern32", 65, 65, 5, 1, KO.WIDE_COLS, False, 0),
	("matern52", 15, 777, 3, 17, None, False, 3),
	("matern12", 64, 63, 12, 1, None, True, 2),
	("se", 5, 2500, 3, 5, None, False, 0),
]
IDS = ["%s-n%d-q%d-d%d-t%d%s%s%s" % (c[0], c[1], c[2], c[3], c[4], "-cols" if c[5] else "", "-coincide" if c[6] else "", "-wideb" if c[7] else "") for c in CASES]
KAPPA = 1.3
_TRUTH = {}


def inputs(ci):
	kind, n, q, d, t, cols, co, wb = CASES[ci]
	rng = np.random.RandomState(9300 + ci)
	a = rng.uniform(-1, 1, size=(n, 8 if cols else d))
	b = rng.uniform(-1, 1, size=(q, 8 if cols else d + wb))
	if co:
		h = max(1, min(n, q) // 2)
		b[:h, :a.shape[1]] = a[:h]
	il = rng.uniform(0.5, 3.0, size=(d,)) / np.sqrt(d)
	V = rng.standard_normal((t, q))
	return tuple(v.astype(np.float32).astype(np.float64) for v in (a, b, il, V))


def truth(ci):
	"""(out, S0, S1, SK) of a case in longdouble, computed once."""
	if ci not in _TRUTH:
		kind, n, q, d, t, cols, co, wb = CASES[ci]
		a, b, il, V = inputs(ci)
		_TRUTH[ci] = PO.kmv_dx_dense(kind, a, b[:, :a.shape[1]], il, V, cols=cols, kappa=KAPPA)
	return _TRUTH[ci]


def device(ci, dtype_name, pad=(0, 0, 0), want_y=False):
	"""out of a case; pad = extra elements of (ldv, ldc in points, ldo).  The padding of out must come back untouched."""
	from stpy_amd import _lib
	kind, n, q, d, t, cols, co, wb = CASES[ci]
	dev, dt = _lib.device(), TORCH[dtype_name]
	a, b, il, V = (torch.from_numpy(v).to(dev, dt) for v in inputs(ci))
	colt = torch.tensor(cols, dtype=torch.int32, device=dev) if cols else None
	Vt = torch.full((t, q + pad[0]), float("nan"), dtype=dt, device=dev)[:, :q]
	Vt.copy_(V)
	store = torch.full((t, n + pad[1], d + 1 + pad[2]), float("nan"), dtype=dt, device=dev)
	out = store[:, :n, :d + 1]
	_lib.kmv_dx(KO.KIND_CODE[kind], a, b, Vt, out, il, cols=colt, kappa=KAPPA)
	Y = None
	if want_y:
		Y = torch.empty((t, n), dtype=dt, device=dev)
		_lib.kmv(KO.KIND_CODE[kind], a, b, Vt, Y, il, cols=colt, kappa=KAPPA)
	torch.cuda.synchronize()
	full = store.cpu().numpy()
	assert np.all(np.isnan(full[:, n:, :])) and np.all(np.isnan(full[:, :, d + 1:]))
	got = full[:, :n, :d + 1].copy()
	return (got, Y.cpu().numpy()) if want_y else got


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_kmv_dx_against_the_longdouble_oracle(ci, dtype_name):
	kind, n, q, d, t, cols, co, wb = CASES[ci]
	want, S0, S1, SK = truth(ci)
	bound = PO.kmv_dx_bound(q, d, KO.eps_of(TORCH_NP[dtype_name]), S0, S1, SK)
	got = device(ci, dtype_name)
	assert got.shape == (t, n, d + 1) and np.all(np.isfinite(got))
	err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
	with np.errstate(divide="ignore", invalid="ignore"):
		ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
	print("%s %s: largest error / bound: gradient columns %.4f, value %.4f" % (IDS[ci], dtype_name, ratio[:, :, :d].max(), ratio[:, :, d].max()))
	assert np.all(err <= bound), (IDS[ci], float(ratio.max()))
	if co and q == 1:
		assert np.all(got[:, 0, :d] == 0)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_kmv_dx_coinciding_points_contribute_exactly_zero(dtype_name):
	"""Every query point IS a contracted point, and nothing else is contracted against it with weight: V is nonzero only on the coinciding
	column, so the gradient is exactly 0 (Matern 1/2: no 0 / 0) and the value is kappa V."""
	from stpy_amd import _lib
	dev, dt = _lib.device(), TORCH[dtype_name]
	rng = np.random.RandomState(5)
	b = torch.from_numpy(rng.uniform(-1, 1, size=(70, 3))).to(dev, dt)
	a = b[:20].clone()
	il = torch.tensor([1.5, 0.75, 2.0], dtype=dt, device=dev)
	for kind in KO.KIND_CODE:
		V = torch.zeros((20, 70), dtype=dt, device=dev)
		V[torch.arange(20), torch.arange(20)] = torch.arange(1, 21, dtype=dt, device=dev)
		out = torch.full((20, 20, 4), float("nan"), dtype=dt, device=dev)
		_lib.kmv_dx(KO.KIND_CODE[kind], a, b, V, out, il, kappa=2.0)
		got = out.cpu().numpy()
		assert np.all(np.isfinite(got)), kind
		for c in range(20):
			assert np.all(got[c, c, :3] == 0), (kind, c)
			assert got[c, c, 3] == 2.0 * (c + 1), (kind, c)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("ci", [2, 4, 5, 7, 9], ids=[IDS[i] for i in (2, 4, 5, 7, 9)])
def test_kmv_dx_same_bits_twice_and_for_padded_leading_dimensions(ci, dtype_name):
	a = device(ci, dtype_name)
	b = device(ci, dtype_name)
	c = device(ci, dtype_name, pad=(11, 5, 3))
	assert np.array_equal(a, b)
	assert np.array_equal(a, c)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("ci", [3, 5, 6, 9], ids=[IDS[i] for i in (3, 5, 6, 9)])
def test_kmv_dx_value_column_agrees_with_stpy_kmv(ci, dtype_name):
	"""out[:, :, d] against stpy_kmv on the same operands: within the sum of both products' bounds."""
	kind, n, q, d, t, cols, co, wb = CASES[ci]
	SK = truth(ci)[3]
	got, Y = device(ci, dtype_name, want_y=True)
	bound = 2 * (2 * KO.eps_of(TORCH_NP[dtype_name]) * (q + d + 8) * SK)
	assert np.all(np.abs(got[:, :, d].astype(np.float64) - Y.astype(np.float64)) <= bound)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_kmv_dx_empty_problems(dtype_name):
	"""n == 0 writes nothing (the raw entry point, handed a buffer it must not touch); q == 0 writes zeros."""
	from stpy_amd import _lib
	dev, dt = _lib.device(), TORCH[dtype_name]
	lib = _lib.load()
	buf = torch.full((3 * 8 * 5,), float("nan"), dtype=dt, device=dev)
	x = torch.zeros((8, 4), dtype=dt, device=dev)
	il = torch.ones(4, dtype=dt, device=dev)
	V = torch.ones((3, 8), dtype=dt, device=dev)
	work = torch.empty((4096,), dtype=torch.uint8, device=dev)
	rc = lib.stpy_kmv_dx(0, _lib.dtype_code(dt), _lib.ptr(x), 0, 4, _lib.ptr(x), 8, 4, 4, None, _lib.ptr(il), 1.0, _lib.ptr(V), 8, 3, _lib.ptr(buf), 40, 5,
						 _lib.ptr(work), work.numel(), _lib.stream_ptr())
	assert rc == 0
	torch.cuda.synchronize()
	assert bool(torch.isnan(buf).all())
	for n in (1, 70):
		store = torch.full((3, n + 2, 7), float("nan"), dtype=dt, device=dev)
		out = store[:, :n, :5]
		_lib.kmv_dx(1, torch.zeros((n, 4), dtype=dt, device=dev), torch.empty((0, 4), dtype=dt, device=dev), torch.empty((3, 0), dtype=dt, device=dev), out, il)
		full = store.cpu().numpy()
		assert np.all(full[:, :n, :5] == 0) and np.all(np.isnan(full[:, n:, :])) and np.all(np.isnan(full[:, :, 5:]))
