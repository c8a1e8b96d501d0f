"""
stpy_kmv on the device: Yt = Vt (K + diag_add I) with K generated on the fly (csrc/kmv.hip), both dtypes, against K @ V of the float64 NumPy
oracle (tests/nystrom_oracle.kernel).

The tolerance is derived per entry, not chosen: 2 eps (q + d + 8) (|K| |V|)_ci -- the kernel-value contract ((d + 8) eps per value) plus the
worst-case summation of q terms, eps that of the dtype; float32 runs get float32-rounded points and vectors, so the oracle sees the same data.
Shapes are the smallest at which each path can break: n of 1, below a wave's 16 points, one past two 64-point tiles, many tiles, past 4096;
t of 1, ragged (3), one full block (16), one past it (17), a full pass (64), one pass and a ragged block (70); d = 1, 2, 5, 12 (the three
register forms, d = 5 with a column subset of a wider x), 20 and 33 (two and three 16-coordinate rounds through LDS); every kind; the two rectangular shapes (n = 5 against
q = 20 000 forces the cut of the j range into 64 pieces; n = 2500 against q = 129 is the uncut walk over three chunks); diag_add on and off.
"""
import numpy as np
import pytest
import torch

from tests import kmv_oracle as KO
from tests import nystrom_oracle as NO

pytestmark = pytest.mark.gpu

WIDE = KO.WIDE_COLS
# (kind, n, q or None for a == b, d, cols, gamma, t, diag_add)
CASES = [
	("se", 1, None, 1, None, 0.3, 1, 0.5),
	("matern12", 15, None, 2, None, 0.5, 3, 0.0),
	("matern32", 129, None, 5, WIDE, 1.0, 16, 0.01),
	("matern52", 777, None, 2, None, 0.5, 17, 0.0),
	("se", 2500, None, 1, None, 0.3, 64, 0.1),
	("matern52", 4099, None, 5, WIDE, 1.0, 70, 0.25),
	("se", 5, 20000, 2, None, 0.5, 3, 0.0),
	("matern32", 2500, 129, 1, None, 0.3, 1, 0.0),
	("se", 777, None, 20, None, 3.0, 5, 0.1),
	("matern12", 300, 777, 12, None, 2.0, 17, 0.0),
	("matern52", 129, 300, 33, None, 4.0, 3, 0.0),
]
IDS = ["%s-n%d-q%s-d%d-t%d" % (c[0], c[1], c[2] or c[1], c[3], c[6]) for c in CASES]
DTYPES = [torch.float64, torch.float32]
KAPPA = 1.5


def np_dtype(dtype):
	return np.float32 if dtype == torch.float32 else np.float64


def case_inputs(idx, dtype):
	kind, n, q, d, cols, gamma, t, diag_add = CASES[idx]
	rng = np.random.RandomState(5200 + idx)
	width = 8 if cols else d
	a = rng.uniform(-1, 1, size=(n, width)).astype(np_dtype(dtype))
	b = a if q is None else rng.uniform(-1, 1, size=(q, width)).astype(np_dtype(dtype))
	V = rng.standard_normal((b.shape[0], t)).astype(np_dtype(dtype))
	return a, b, V


def run_device(kind, a, b, V, gamma, cols=None, diag_add=0.0, kappa=KAPPA, pad=0, same=False):
	"""Yt (t, n) of the device for V (q, t); pad: extra elements in the row strides of Vt and Yt."""
	from stpy_amd import _lib
	dev = _lib.device()
	ad = torch.from_numpy(a).to(dev)
	bd = ad if same else torch.from_numpy(b).to(dev)
	d = len(cols) if cols else a.shape[1]
	inv_ls = torch.full((d,), 1.0 / gamma, dtype=ad.dtype, device=dev)
	cd = torch.tensor(cols, dtype=torch.int32, device=dev) if cols else None
	q, t = V.shape
	Vt = torch.full((t, q + pad), float("nan"), dtype=ad.dtype, device=dev)[:, :q]
	Vt.copy_(torch.from_numpy(np.ascontiguousarray(V.T)))
	Yt = torch.full((t, a.shape[0] + pad), float("nan"), dtype=ad.dtype, device=dev)[:, :a.shape[0]]
	_lib.kmv(KO.KIND_CODE[kind], ad, bd, Vt, Yt, inv_ls, cols=cd, kappa=kappa, diag_add=diag_add)
	torch.cuda.synchronize()
	return Yt.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_kmv_against_dense_product(idx, dtype):
	kind, n, q, d, cols, gamma, t, diag_add = CASES[idx]
	a, b, V = case_inputs(idx, dtype)
	Yt = run_device(kind, a, b, V, gamma, cols, diag_add, same=q is None)
	a64, b64, V64 = a.astype(np.float64), b.astype(np.float64), V.astype(np.float64)
	ref, mag = KO.kmv_bound(kind, a64, b64, gamma, V64, cols, KAPPA)
	if diag_add:
		ref = ref + diag_add * V64
		mag = mag + abs(diag_add) * np.abs(V64)
	eps = KO.eps_of(np_dtype(dtype))
	bound = 2 * eps * (b.shape[0] + d + 8) * mag
	err = np.abs(Yt.T.astype(np.float64) - ref)
	print("%s %s: largest error / bound %.3g" % (IDS[idx], dtype, float((err / np.maximum(bound, 1e-300)).max())))
	assert np.all(np.isfinite(Yt))
	assert np.all(err <= bound)
	# determinism: a second call gives the same bits, and so does a padded row stride of Vt and Yt
	assert np.array_equal(run_device(kind, a, b, V, gamma, cols, diag_add, same=q is None), Yt)
	assert np.array_equal(run_device(kind, a, b, V, gamma, cols, diag_add, pad=3, same=q is None), Yt)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", NO.KINDS)
def test_kmv_identity_gives_a_bitwise_symmetric_matrix(kind, dtype):
	"""Vt = I at n = q = 129 (three passes of right-hand sides): the output is K + diag_add I itself, bitwise symmetric, exactly kappa + diag_add
	on the diagonal, and within the kernel-value contract of the oracle's matrix."""
	n, d, gamma, diag_add = 129, 2, 0.5, 0.25
	a = np.random.RandomState(61).uniform(-1, 1, size=(n, d)).astype(np_dtype(dtype))
	Yt = run_device(kind, a, a, np.eye(n, dtype=np_dtype(dtype)), gamma, None, diag_add, same=True)
	assert np.array_equal(Yt, Yt.T)
	assert np.all(np.diag(Yt) == np_dtype(dtype)(KAPPA + diag_add))
	K = NO.kernel(kind, a.astype(np.float64), a.astype(np.float64), gamma, KAPPA) + diag_add * np.eye(n)
	assert np.abs(Yt - K).max() <= 2 * KO.eps_of(np_dtype(dtype)) * (d + 8) * KAPPA
	# ... and without the diagonal term, the rectangular entry point on the same points gives the same off-diagonal bits
	Y0 = run_device(kind, a, a, np.eye(n, dtype=np_dtype(dtype)), gamma, None, 0.0, same=False)
	off = ~np.eye(n, dtype=bool)
	assert np.array_equal(Y0[off], Yt[off]) and np.all(np.diag(Y0) == np_dtype(dtype)(KAPPA))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_kmv_duplicated_points_give_equal_rows(dtype):
	"""40 distinct points eight times each, shuffled (n = 320, the j range cut into pieces): copies of a point get bit-equal outputs."""
	rng = np.random.RandomState(62)
	base = rng.uniform(-1, 1, size=(40, 3)).astype(np_dtype(dtype))
	owner = rng.permutation(np.repeat(np.arange(40), 8))
	a = base[owner]
	V = rng.standard_normal((320, 6)).astype(np_dtype(dtype))
	Yt = run_device("matern52", a, a, V, 0.7, None, 0.0, same=True)
	first = np.array([np.flatnonzero(owner == o)[0] for o in owner])
	assert np.array_equal(Yt, Yt[:, first])


def test_kmv_empty_contraction_writes_zeros():
	a = np.random.RandomState(63).uniform(-1, 1, size=(70, 2))
	Yt = run_device("se", a, np.zeros((0, 2)), np.zeros((0, 3)), 0.5)
	assert Yt.shape == (3, 70) and np.all(Yt == 0)
