"""
stpy_pchol on the device: greedy pivoted partial Cholesky of an on-the-fly kernel matrix (csrc/pchol.hip), both dtypes.

Pivot lists are NOT compared with the oracle's own pivots: near-ties between the two largest residuals (relative gaps down to 1e-16) make the
greedy choice a matter of the last bit.  Instead, with the kernel's own pivots forced into the float64 NumPy oracle ("replay"):
  1. validity      rank = m, pivots distinct and in range, piv[0] = 0 (the lowest index of the all-equal start);
  2. factor        Ft and dres against the replay: fp64 at the project's 1e-8 absolute (kappa = 1); fp32 at 8 x the error the oracle's OWN
                   float32 replay makes against the float64 replay on that case (floor 16 eps32) -- computed per case, never a fixed number;
                   the factor 8 covers the hardware's exp and a different summation order, which share the oracle's (j eps) growth;
  3. greediness    at EVERY step the replay's residual at piv[j] is within that same tolerance of the replay's largest residual;
  4. determinism   two calls are bit-identical; a padded row stride (the 16-byte loads with a ragged last lane) gives the same bits;
  5. early stop    10 distinct points five times each: rank 10, zero rows and -1 pivots after it, no pivot on a copy of an earlier one;
  6. error figure  NystromFeatures.trace_error = trace(K) - |F|_F^2 of the replay, to the tolerance of item 2 times n.
Data: uniform(-1, 1) from a fixed seed per case; the float32 runs get the float32-rounded points, and so do their replays.

The cases are the issue's; the last two are added for code paths the others do not reach: m above 1024 (the values Ft[0:j, p] pass through
LDS in chunks of 1024), and the decaying 1-D case whose m = 12 the oracle chose (its last pivot is 2.3e-4 in float64 and 5.8e-4 in float32, between 1e-4 and 1e-2).
"""
import numpy as np
import pytest
import torch

from tests import nystrom_oracle as NO

pytestmark = pytest.mark.gpu

KIND_CODE = {"se": 0, "matern12": 1, "matern32": 2, "matern52": 3}
WIDE_COLS = [6, 1, 3, 0, 5]
# (kind, n, d, gamma, m, coordinates read from a wider x or None)
CASES = [
	("se", 777, 2, 0.35, 33, None),
	("se", 2500, 3, 0.25, 130, None),
	("matern52", 4099, 2, 0.1, 64, None),
	("matern12", 1000, 5, 0.8, 40, WIDE_COLS),
	("matern32", 1, 1, 0.5, 1, None),
	("se", 300, 1, 0.05, 24, None),
	("se", 300, 1, 0.3, 12, None),
	("matern12", 1300, 5, 0.3, 1100, None),
]
IDS = ["%s-n%d-d%d-m%d" % (c[0], c[1], c[2], c[4]) for c in CASES]
DTYPES = [torch.float64, torch.float32]
EPS32 = float(np.finfo(np.float32).eps)


def case_points(idx, dtype):
	kind, n, d, gamma, m, cols = CASES[idx]
	x = np.random.RandomState(4100 + idx).uniform(-1, 1, size=(n, 8 if cols else d))
	return x.astype(np.float32) if dtype == torch.float32 else x


def run_device(kind, x, gamma, m, cols=None, tol=0.0, ldf=None):
	from stpy_amd import _lib
	xd = torch.from_numpy(x).to(_lib.device())
	d = len(cols) if cols else x.shape[1]
	inv_ls = torch.full((d,), 1.0 / gamma, dtype=xd.dtype, device=xd.device)
	cd = torch.tensor(cols, dtype=torch.int32, device=xd.device) if cols else None
	piv, Ft, dres, rank = _lib.pchol(KIND_CODE[kind], xd, inv_ls, m, cols=cd, kappa=1.0, tol=tol, ldf=ldf)
	torch.cuda.synchronize()
	return piv, Ft, dres, rank


_RESULTS = {}


def result(idx, dtype):
	"""One device run and one float64 replay (plus the float32 replay for the fp32 tolerance) per case and dtype, shared by the tests."""
	key = (idx, dtype)
	if key not in _RESULTS:
		kind, n, d, gamma, m, cols = CASES[idx]
		x = case_points(idx, dtype)
		piv, Ft, dres, rank = run_device(kind, x, gamma, m, cols)
		out = dict(piv=piv.cpu().numpy(), Ft=Ft.cpu().numpy(), dres=dres.cpu().numpy(), rank=int(rank.item()), dev=(piv, Ft, dres, rank), x=x)
		pv = out["piv"]
		ok = out["rank"] == m and pv.min() >= 0 and pv.max() < n and len(set(pv.tolist())) == m
		out["valid"] = ok
		if ok:
			tr = []
			_, F64, d64, _ = NO.pivoted_cholesky(kind, x.astype(np.float64), gamma, m, cols=cols, pivots=pv, trace=tr)
			out.update(F64=F64, d64=d64, trace=tr, tol=1e-8)
			if dtype == torch.float32:
				_, F32, d32, _ = NO.pivoted_cholesky(kind, x, gamma, m, cols=cols, pivots=pv, dtype=np.float32)
				own = max(np.abs(F32 - F64).max(), np.abs(d32 - d64).max())
				out.update(own=own, tol=max(8.0 * own, 16.0 * EPS32))
		_RESULTS[key] = out
	return _RESULTS[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_validity(idx, dtype):
	r = result(idx, dtype)
	m, n = CASES[idx][4], CASES[idx][1]
	pv = r["piv"]
	assert r["rank"] == m
	assert pv.min() >= 0 and pv.max() < n and len(set(pv.tolist())) == m
	assert pv[0] == 0
	assert np.all(r["dres"][pv] == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_factor_matches_replay(idx, dtype):
	r = result(idx, dtype)
	assert r["valid"]
	eF, ed = np.abs(r["Ft"] - r["F64"]).max(), np.abs(r["dres"] - r["d64"]).max()
	print("case %s %s: |Ft - replay| %.3e  |dres - replay| %.3e  tolerance %.3e%s" % (
		IDS[idx], dtype, eF, ed, r["tol"], "  (oracle's own float32 replay %.3e)" % r["own"] if "own" in r else ""))
	assert eF <= r["tol"] and ed <= r["tol"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_greedy_at_every_step(idx, dtype):
	r = result(idx, dtype)
	assert r["valid"]
	assert len(r["trace"]) == CASES[idx][4]
	worst = max(top - at for at, top in r["trace"])
	print("case %s %s: largest shortfall of a pivot against the step's maximum %.3e (slack %.3e); last pivot %.3e" % (
		IDS[idx], dtype, worst, r["tol"], r["trace"][-1][0]))
	for j, (at, top) in enumerate(r["trace"]):
		assert at >= top - r["tol"], (j, at, top)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idx", [0, 1, 3, 7], ids=[IDS[i] for i in (0, 1, 3, 7)])
def test_two_calls_are_bit_identical(idx, dtype):
	r = result(idx, dtype)
	kind, n, d, gamma, m, cols = CASES[idx]
	again = run_device(kind, r["x"], gamma, m, cols)
	for a, b in zip(r["dev"], again):
		assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_padded_row_stride_gives_the_same_bits(dtype):
	"""n = 777 with ldf = n takes the element-wise loads (rows not 16-byte aligned), ldf = 780 the 16-byte loads with a last lane that
	holds fewer than V points: same sums in the same order."""
	r = result(0, dtype)
	kind, n, d, gamma, m, cols = CASES[0]
	padded = run_device(kind, r["x"], gamma, m, cols, ldf=780)
	assert padded[1].stride(0) == 780
	for a, b in zip(r["dev"], padded):
		assert torch.equal(a, b)


def _duplicated_points(dtype):
	rng = np.random.RandomState(77)
	x = np.repeat(rng.uniform(-1, 1, size=(10, 2)), 5, axis=0)[rng.permutation(50)]
	return x.astype(np.float32) if dtype == torch.float32 else x


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_early_stop_on_duplicates(dtype):
	"""SE, gamma = 0.5, 10 distinct points five times each, shuffled.  Oracle: the tenth pivot is 2.7e-2 and the largest residual after it
	3.9e-16 (float64) / 6.0e-8 (float32), so tol = 1e-10 / 1e-4 separates the two by orders of magnitude on either side."""
	x = _duplicated_points(dtype)
	tol = 1e-10 if dtype == torch.float64 else 1e-4
	np_dt = np.float64 if dtype == torch.float64 else np.float32
	tr = []
	_, _, dres_o, rank_o = NO.pivoted_cholesky("se", x, 0.5, 16, tol=tol, dtype=np_dt, trace=tr)
	print("oracle: tenth pivot %.3e, largest residual after it %.3e" % (tr[9][0], tr[10][1]))
	assert rank_o == 10 and tr[9][0] > 100 * tol and tr[10][1] < tol / 100
	piv, Ft, dres, rank = run_device("se", x, 0.5, 16, tol=tol)
	piv, Ft, dres = piv.cpu().numpy(), Ft.cpu().numpy(), dres.cpu().numpy()
	assert int(rank.item()) == 10
	assert np.all(Ft[10:] == 0) and np.all(piv[10:] == -1)
	assert piv[:10].min() >= 0 and piv[:10].max() < 50
	assert len({tuple(x[p]) for p in piv[:10]}) == 10          # no pivot indexes a copy of an earlier one
	assert np.abs(dres).max() <= tol and np.all(dres[piv[:10]] == 0)
	# tol = 0 on the same data: the stop is then "not positive" or the cap m, never a repeated pivot
	piv0, _, _, rank0 = run_device("se", x, 0.5, 16, tol=0.0)
	r0 = int(rank0.item())
	p0 = piv0.cpu().numpy()
	assert 10 <= r0 <= 16 and len(set(p0[:r0].tolist())) == r0 and np.all(p0[r0:] == -1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idx", [0, 2], ids=[IDS[0], IDS[2]])
def test_trace_error_of_the_class(idx, dtype):
	from stpy_amd import KernelFunction, NystromFeatures, pivoted_cholesky
	kind, n, d, gamma, m, cols = CASES[idx]
	r = result(idx, dtype)
	assert r["valid"]
	kernel = KernelFunction(kernel_name="squared_exponential", gamma=gamma, d=d) if kind == "se" else KernelFunction(kernel_name="matern", gamma=gamma, nu=2.5, d=d)
	x = torch.from_numpy(r["x"])
	nys = NystromFeatures(kernel, m=m, approx="pivoted", s=0.1)
	nys.fit_gp(x, torch.zeros(n, 1, dtype=x.dtype))
	assert np.array_equal(np.asarray(nys.C), r["piv"])                  # the class runs the same factorisation
	want = n * 1.0 - float(np.sum(r["F64"] * r["F64"]))                 # trace(K) - |F|_F^2, kappa = 1
	got = float(nys.trace_error)
	print("case %s %s: trace_error %.10e, oracle %.10e, tolerance %.3e" % (IDS[idx], dtype, got, want, r["tol"] * n))
	assert abs(got - want) <= r["tol"] * n
	# the module function returns the same factor, (n, r), where x lives
	piv, F, dres, rank = pivoted_cholesky(kernel, x, m)
	assert rank == m and tuple(F.shape) == (n, m) and not F.is_cuda
	assert np.array_equal(piv.numpy(), r["piv"]) and np.array_equal(F.numpy(), r["Ft"].T) and np.array_equal(dres.numpy(), r["dres"])
