"""
stpy_kmv_dxx on the device (csrc/kmvdxx.hip) against the longdouble statement of tests/kmv_dxx_oracle.py, within its bounds: the stpy_kmv_dx
bound on the gradient and value columns, 2 eps (q + d + 12) SH on the Hessian block (SH the sum of magnitudes of its two parts;
tests/test_kmv_dxx_cpu.py shows a working-precision emulation inside the bound).  Inputs are rounded to float32 so that one truth serves both
types.  The cross product n in {1, 15, 17, 65} x q in {1, 63, 65, 300} with d cycling through {1, 3, 4, 5, 8, 9, 16} (every instantiation, odd
and even d: a middle Hessian row alone in its group) and t through {1, 3, 16, 17}; strict subsets ``cols`` of a width-8 x with distinct,
non-monotone inv_ls; n = 5 against q = 1000, whose j range is cut into pieces; coinciding points; empty problems; the same bits twice, for
padded leading dimensions, and for an integer translate of dyadic data (the evaluator's contract, layouts of tests/direct_eval_cases.py).
"""
import numpy as np
import pytest
import torch

from tests import direct_eval_cases as D
from tests import kmv_oracle as KO
from tests import kmv_dxx_oracle as XO
from tests import pathwise_oracle as PO

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
TORCH = {"float64": torch.float64, "float32": torch.float32}
TORCH_NP = {"float64": np.float64, "float32": np.float32}
NS, QS, DS, TS = (1, 15, 17, 65), (1, 63, 65, 300), (1, 3, 4, 5, 8, 9, 16), (1, 3, 16, 17)
# (kind, n, q, d, t, cols on a width-8 x, coinciding points)
CASES = []
for _ni, _n in enumerate(NS):
	for _qi, _q in enumerate(QS):
		_i = len(CASES)
		CASES.append((XO.HESSIAN_KINDS[(_ni + _i) % 2], _n, _q, DS[_i % len(DS)], TS[(_ni + _qi) % len(TS)], None, _i % 5 == 2))
SPLIT = len(CASES)
CASES += [
	("se", 5, 1000, 3, 5, None, False),                     # the j range is cut into pieces
	("matern52", 5, 1000, 16, 1, None, True),
	("matern52", 17, 300, 5, 3, KO.WIDE_COLS, False),       # a strict, non-monotone subset of a wider x
	("se", 65, 65, 3, 17, [6, 1, 3], True),
	("se", 15, 63, 16, 16, None, False),
	("matern52", 65, 300, 9, 17, None, False),
]
IDS = ["%s-n%d-q%d-d%d-t%d%s%s" % (c[0], c[1], c[2], c[3], c[4], "-cols" if c[5] else "", "-coincide" if c[6] else "") for c in CASES]
KAPPA = 1.3
_TRUTH = {}


def test_the_cases_cover_what_they_claim():
	assert {c[1] for c in CASES} >= set(NS) and {c[2] for c in CASES} >= set(QS) and {c[3] for c in CASES} == set(DS) and {c[4] for c in CASES} >= set(TS)
	assert {(c[1], c[2]) for c in CASES} >= {(n, q) for n in NS for q in QS}
	for kind in XO.HESSIAN_KINDS:
		assert {4 if c[3] <= 4 else 8 if c[3] <= 8 else 16 for c in CASES if c[0] == kind} == {4, 8, 16}          # every instantiation
	for c in CASES:
		if c[5]:
			assert len(c[5]) == c[3] < 8 and sorted(c[5]) != list(c[5])
		il = inputs(CASES.index(c))[2]
		assert len(set(il)) == c[3] and (c[3] < 3 or (np.any(np.diff(il) > 0) and np.any(np.diff(il) < 0)))


def inputs(ci):
	kind, n, q, d, t, cols, co = CASES[ci]
	rng = np.random.RandomState(9700 + ci)
	a = rng.uniform(-1, 1, size=(n, 8 if cols else d))
	b = rng.uniform(-1, 1, size=(q, 8 if cols else d))
	if co:
		h = max(1, min(n, q) // 2)
		b[:h] = a[:h]
	while True:
		il = rng.uniform(0.5, 3.0, size=(d,)) / np.sqrt(d)
		if d < 3 or (np.any(np.diff(il) > 0) and np.any(np.diff(il) < 0)):
			break
	V = rng.standard_normal((t, q))
	return tuple(v.astype(np.float32).astype(np.float64) for v in (a, b, il, V))


def truth(ci):
	"""(out, S0, S1, SK, SH) of a case in longdouble, computed once."""
	if ci not in _TRUTH:
		kind, n, q, d, t, cols, co = CASES[ci]
		a, b, il, V = inputs(ci)
		_TRUTH[ci] = XO.kmv_dxx_dense(kind, a, b, il, V, cols=cols, kappa=KAPPA)
	return _TRUTH[ci]


def run(kind, a, b, il, V, cols, dtype_name, pad=(0, 0, 0), kappa=KAPPA, want_dx=False):
	"""stpy_kmv_dxx on host arrays; pad = extra elements of (ldv, ldc in points, ldo).  The padding of out must come back untouched."""
	from stpy_amd import _lib
	dev, dt = _lib.device(), TORCH[dtype_name]
	n, q, t, d = a.shape[0], b.shape[0], V.shape[0], len(il)
	nc = XO.ncol(d)
	a, b, il, V = (torch.from_numpy(np.ascontiguousarray(v)).to(dev, dt) for v in (a, b, il, V))
	colt = torch.tensor(cols, dtype=torch.int32, device=dev) if cols else None
	Vt = torch.full((t, q + pad[0]), float("nan"), dtype=dt, device=dev)[:, :q]
	Vt.copy_(V)
	store = torch.full((t, n + pad[1], nc + pad[2]), float("nan"), dtype=dt, device=dev)
	_lib.kmv_dxx(KO.KIND_CODE[kind], a, b, Vt, store[:, :n, :nc], il, cols=colt, kappa=kappa)
	first = None
	if want_dx:
		first = torch.empty((t, n, d + 1), dtype=dt, device=dev)
		_lib.kmv_dx(KO.KIND_CODE[kind], a, b, Vt, first, il, cols=colt, kappa=kappa)
	torch.cuda.synchronize()
	full = store.cpu().numpy()
	assert np.all(np.isnan(full[:, n:, :])) and np.all(np.isnan(full[:, :, nc:]))
	got = full[:, :n, :nc].copy()
	return (got, first.cpu().numpy()) if want_dx else got


def device(ci, dtype_name, pad=(0, 0, 0), want_dx=False):
	kind, n, q, d, t, cols, co = CASES[ci]
	a, b, il, V = inputs(ci)
	return run(kind, a, b, il, V, cols, dtype_name, pad, want_dx=want_dx)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_kmv_dxx_against_the_longdouble_oracle(ci, dtype_name):
	kind, n, q, d, t, cols, co = CASES[ci]
	want, S0, S1, SK, SH = truth(ci)
	eps = KO.eps_of(TORCH_NP[dtype_name])
	bound = XO.kmv_dxx_bound(q, d, eps, S0, S1, SK, SH)
	got, first = device(ci, dtype_name, want_dx=True)
	assert got.shape == (t, n, XO.ncol(d)) and np.all(np.isfinite(got))
	err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
	with np.errstate(divide="ignore", invalid="ignore"):
		ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
	print("%s %s: largest error / bound: gradient %.4f, value %.4f, Hessian %.4f" % (IDS[ci], dtype_name, ratio[:, :, :d].max(), ratio[:, :, d].max(), ratio[:, :, d + 1:].max()))
	assert np.all(err <= bound), (IDS[ci], float(ratio.max()))
	# the first d + 1 columns against stpy_kmv_dx's own output on the same operands: within stpy_kmv_dx's bound
	assert np.all(np.abs(got[:, :, :d + 1].astype(np.float64) - first.astype(np.float64)) <= PO.kmv_dx_bound(q, d, eps, S0, S1, SK))


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_kmv_dxx_cuts_the_j_range_of_few_queries_against_many_points(dtype_name):
	"""n = 5 against q = 1000: the workspace query asks for room for at least two pieces' tiles (it asks for nothing where the range is whole),
	so the cases at SPLIT and SPLIT + 1 above went through the second launch."""
	from stpy_amd import _lib
	lib, code, esz = _lib.load(), (0 if dtype_name == "float64" else 1), (8 if dtype_name == "float64" else 4)
	for ci in (SPLIT, SPLIT + 1):
		kind, n, q, d, t, cols, co = CASES[ci]
		assert (n, q) == (5, 1000)
		assert lib.stpy_kmv_dxx_workspace_bytes(code, n, q, d, t) >= 2 * t * n * XO.ncol(d) * esz
		assert lib.stpy_kmv_dxx_workspace_bytes(code, n, 256, d, t) <= 512


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_kmv_dxx_coinciding_points_contribute_exactly_the_diagonal(dtype_name):
	"""Every query point IS a contracted point and V is nonzero only on the coinciding column: the gradient is exactly 0, the value kappa V and
	the Hessian exactly kappa chi(0) il_k^2 V [k == l] (chi(0) = -1 for SE, -5/3 for Matern 5/2; V, kappa and inv_ls are powers of two or
	short dyadics, so no product below rounds)."""
	from stpy_amd import _lib
	T = TORCH_NP[dtype_name]
	rng = np.random.RandomState(5)
	b = rng.uniform(-1, 1, size=(70, 3)).astype(np.float32).astype(np.float64)
	a = b[:20].copy()
	il = np.array([1.5, 0.75, 2.0])
	V = np.zeros((20, 70))
	V[np.arange(20), np.arange(20)] = 2.0 ** (np.arange(20) % 5)
	for kind, chi0 in (("se", T(-1.0)), ("matern52", T(-5.0 / 3.0))):
		got = run(kind, a, b, il, V, None, dtype_name, kappa=2.0)
		assert got.dtype == T and np.all(np.isfinite(got)), kind
		for c in range(20):
			assert np.all(got[c, c, :3] == 0), (kind, c)
			assert got[c, c, 3] == 2.0 * V[c, c], (kind, c)
			H = XO.full_hessian(got[c, c, 4:], 3)
			want = np.diag((T(2.0) * chi0 * T(V[c, c])) * (il * il).astype(T))
			assert np.array_equal(H, want), (kind, c, H, want)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("ci", [5, 10, SPLIT, SPLIT + 1, SPLIT + 2, SPLIT + 4], ids=[IDS[i] for i in (5, 10, SPLIT, SPLIT + 1, SPLIT + 2, SPLIT + 4)])
def test_kmv_dxx_same_bits_twice_and_for_padded_leading_dimensions(ci, dtype_name):
	a = device(ci, dtype_name)
	b = device(ci, dtype_name)
	c = device(ci, dtype_name, pad=(11, 5, 3))
	assert np.array_equal(a, b)
	assert np.array_equal(a, c)
	# lda / ldb: the same points as columns of wider storage
	kind, n, q, d, t, cols, co = CASES[ci]
	if cols is None:
		xa, xb, il, V = inputs(ci)
		wa, wb = np.full((n, d + 3), 7.0), np.full((q, d + 2), -3.0)
		wa[:, :d], wb[:, :d] = xa, xb
		e = run(kind, wa, wb, il, V, list(range(d)), dtype_name)
		assert np.array_equal(a, e)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("shift", ["offset", "offset_per_column"])
@pytest.mark.parametrize("d", [3, 8, 16])
def test_kmv_dxx_integer_translate_of_dyadic_data_changes_no_bit(d, shift, dtype_name):
	"""The evaluator's contract (difference first, scale second): a dyadic layout and its translate by integers have exactly the same coordinate
	differences, so every output has the same bits."""
	dt = "f64" if dtype_name == "float64" else "f32"
	case = D.ard_case("cube", d, dt, 17, 130)
	moved = D.twin(case, shift)
	V = np.random.RandomState(77 + d).standard_normal((3, 130)).astype(np.float32).astype(np.float64)
	for kind in XO.HESSIAN_KINDS:
		here = run(kind, case.a, case.b, case.inv_ls, V, None, dtype_name)
		there = run(kind, moved.a, moved.b, moved.inv_ls, V, None, dtype_name)
		assert np.any(here[:, :, d + 1:] != 0) and np.array_equal(here, there), (kind, d, shift)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_kmv_dxx_empty_problems(dtype_name):
	"""n == 0 writes nothing (the raw entry point, handed a buffer it must not touch); q == 0 writes zeros."""
	from stpy_amd import _lib
	dev, dt = _lib.device(), TORCH[dtype_name]
	lib = _lib.load()
	nc = XO.ncol(4)
	buf = torch.full((3 * 8 * nc,), float("nan"), dtype=dt, device=dev)
	x = torch.zeros((8, 4), dtype=dt, device=dev)
	il = torch.ones(4, dtype=dt, device=dev)
	V = torch.ones((3, 8), dtype=dt, device=dev)
	work = torch.empty((4096,), dtype=torch.uint8, device=dev)
	rc = lib.stpy_kmv_dxx(0, _lib.dtype_code(dt), _lib.ptr(x), 0, 4, _lib.ptr(x), 8, 4, 4, None, _lib.ptr(il), 1.0, _lib.ptr(V), 8, 3, _lib.ptr(buf), 8 * nc, nc,
						  _lib.ptr(work), work.numel(), _lib.stream_ptr())
	assert rc == 0
	torch.cuda.synchronize()
	assert bool(torch.isnan(buf).all())
	for n in (1, 70):
		store = torch.full((3, n + 2, nc + 2), float("nan"), dtype=dt, device=dev)
		out = store[:, :n, :nc]
		_lib.kmv_dxx(3, torch.zeros((n, 4), dtype=dt, device=dev), torch.empty((0, 4), dtype=dt, device=dev), torch.empty((3, 0), dtype=dt, device=dev), out, il)
		full = store.cpu().numpy()
		assert np.all(full[:, :n, :nc] == 0) and np.all(np.isnan(full[:, n:, :])) and np.all(np.isnan(full[:, :, nc:]))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("with_cols", [False, True], ids=["plain", "cols"])
@pytest.mark.parametrize("kind", XO.HESSIAN_KINDS)
@pytest.mark.parametrize("d", [3, 8, 16])
@pytest.mark.parametrize("t", [3, 17])
def test_kmv_dxx_first_columns_are_kmv_dx_bit_for_bit(t, d, kind, with_cols, dtype_name):
	"""With a j range that is never cut (q <= 256) the d gradient columns and the value column of stpy_kmv_dxx ARE the output of stpy_kmv_dx on
	the same operands: group 0 of the kernel is the arithmetic of stpy_kmv_dx, statement for statement.  n = 70 is a ragged tile, q = 200 a
	ragged chunk; every register instantiation, one and two row blocks, coordinates taken directly and through a non-monotone ``cols``."""
	n, q = 70, 200
	rng = np.random.RandomState(4100 + 37 * d + t)
	width = d + 3 if with_cols else d
	cols = [int(c) for c in rng.permutation(width)[:d]] if with_cols else None
	a = rng.uniform(-1, 1, size=(n, width)).astype(np.float32).astype(np.float64)
	b = rng.uniform(-1, 1, size=(q, width)).astype(np.float32).astype(np.float64)
	b[:9] = a[:9]                                                        # rho == 0 pairs
	il = (rng.uniform(0.5, 3.0, size=(d,)) / np.sqrt(d)).astype(np.float32).astype(np.float64)
	V = rng.standard_normal((t, q)).astype(np.float32).astype(np.float64)
	assert cols is None or sorted(cols) != cols
	got, first = run(kind, a, b, il, V, cols, dtype_name, want_dx=True)
	assert first.shape == (t, n, d + 1) and np.all(np.isfinite(first)) and np.any(first[:, :, :d] != 0)
	assert np.array_equal(got[:, :, :d + 1], first)
