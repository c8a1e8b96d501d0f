"""
stpy_pcg on the device: block preconditioned CG on the matrix-free operator of stpy_kmv (csrc/kmv.hip), both dtypes, against the NumPy
restatement in tests/kmv_oracle.py.  Cases: uniform(-1, 1) points from a fixed seed, right-hand sides y and five columns k(x, xt_j); float64
with s = 0.1, tol = 1e-8 and float32 with s = 0.3, tol = 1e-4.  The preconditioner G is the oracle's (computed in the working dtype and
uploaded), so that this file tests the solver alone.

  residual     the TRUE relative residual of the device's X, computed by the float64 oracle, is <= 2 tol: the factor 2 is the room for the gap
               between the recurrence residual the solver stops on and the true one (float64: about eps x iterations x cond ~ 4e-10 here;
               float32: the oracle's own float32 run stays under tol, tests/test_kmv_cpu.py);
  iterations   the device's preconditioned count is at most the geometric mean of the oracle's preconditioned and plain counts of the case: a
               per-case number that a solver which did not apply the preconditioner would miss.  Asserted where the oracle's ratio
               preconditioned / plain is below 0.5, printed otherwise (matern12 1000: 0.66 in float64, 0.56 in float32);
  resumption, freezing, the zero column, bx, r = 0 and the curvature flag as stated at each test.
"""
import numpy as np
import pytest
import torch

from tests import kmv_oracle as KO

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
TORCH = {"float64": torch.float64, "float32": torch.float32}


class Solver:
	"""One stpy_pcg problem on the device: the operands, the state and the outputs; ``run`` enqueues iterations."""

	def __init__(self, kind, x, gamma, B, dtype_name, diag_add, G=None, cols=None, tol=0.0, pad=0):
		from stpy_amd import _lib
		self.L, dev, dt = _lib, _lib.device(), TORCH[dtype_name]
		self.kind = KO.KIND_CODE[kind]
		self.x = torch.from_numpy(x).to(dev, dt)
		d = len(cols) if cols else x.shape[1]
		self.inv_ls = torch.full((d,), 1.0 / gamma, dtype=dt, device=dev)
		self.cols = torch.tensor(cols, dtype=torch.int32, device=dev) if cols else None
		n, t = B.shape
		self.Bt = torch.from_numpy(np.ascontiguousarray(B.T)).to(dev, dt)
		self.Xt = torch.full((t, n + pad), float("nan"), dtype=dt, device=dev)[:, :n]
		self.Gn = self.Gt = None
		if G is not None:
			self.Gn = torch.from_numpy(np.ascontiguousarray(G)).to(dev, dt)
			self.Gt = self.Gn.t().contiguous()
		self.diag_add, self.tol = diag_add, tol
		self.work = _lib.pcg_workspace(n, d, t, 0 if G is None else G.shape[1], self.x)
		self.out = (torch.empty(t, dtype=dt, device=dev), torch.empty(t, dtype=dt, device=dev), torch.empty(t, dtype=torch.int32, device=dev))
		self.started = False

	def run(self, iters):
		self.L.pcg(self.kind, self.x, self.inv_ls, self.Bt, self.Xt, self.work, self.out, cols=self.cols, kappa=1.0, diag_add=self.diag_add,
				   Gt=self.Gt, Gn=self.Gn, tol=self.tol, iters=iters, init=not self.started)
		self.started = True
		torch.cuda.synchronize()
		return self

	def solve(self, block=10, maxiter=3000):
		done = 0
		while done < maxiter:
			self.run(block)
			done += block
			rel, its = self.out[0].cpu().numpy(), self.out[2].cpu().numpy()
			if np.all((rel <= self.tol) | (its < 0)):
				break
		return self

	def get(self):
		return dict(X=self.Xt.cpu().numpy().T.copy(), relres=self.out[0].cpu().numpy(), bx=self.out[1].cpu().numpy(), its=self.out[2].cpu().numpy())


def case_solver(idx, dtype_name, precond=True, **kw):
	kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
	o = KO.oracle_run(idx, dtype_name)
	return Solver(kind, o["x"], gamma, o["B64"], dtype_name, o["s"] ** 2, G=o["G"] if precond else None, cols=cols, tol=o["tol"], **kw)


_SOLVED = {}


def solved(idx, dtype_name):
	if (idx, dtype_name) not in _SOLVED:
		_SOLVED[(idx, dtype_name)] = case_solver(idx, dtype_name).solve().get()
	return _SOLVED[(idx, dtype_name)]


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("idx", range(len(KO.PCG_CASES)), ids=KO.PCG_IDS)
def test_pcg_residual_and_iterations(idx, dtype_name):
	o, got = KO.oracle_run(idx, dtype_name), solved(idx, dtype_name)
	true = KO.true_relres(o["A64"], o["B64"], got["X"])
	its, pre, plain = int(got["its"].max()), int(o["its"].max()), int(o["its_plain"].max())
	print("%s %s: true residual / tol %.3f, recurrence %.3f; iterations %d (oracle %d preconditioned, %d plain, geometric mean %.1f)" % (
		KO.PCG_IDS[idx], dtype_name, true.max() / o["tol"], got["relres"].max() / o["tol"], its, pre, plain, np.sqrt(pre * plain)))
	assert np.all(np.isfinite(got["X"])) and np.all(got["its"] > 0)
	assert np.all(got["relres"] <= o["tol"])
	assert np.all(true <= 2 * o["tol"])
	if pre / plain < 0.5:
		assert its <= np.sqrt(pre * plain)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("idx", [0, 5], ids=[KO.PCG_IDS[0], KO.PCG_IDS[5]])
def test_pcg_bx_is_the_dot_product_of_the_returned_x(idx, dtype_name):
	o, got = KO.oracle_run(idx, dtype_name), solved(idx, dtype_name)
	B, X = o["B64"], got["X"].astype(np.float64)
	eps, n = KO.eps_of(got["X"].dtype), B.shape[0]
	assert np.all(np.abs(got["bx"] - np.sum(B * X, axis=0)) <= 2 * eps * n * np.sum(np.abs(B) * np.abs(X), axis=0))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("idx", [0, 5], ids=[KO.PCG_IDS[0], KO.PCG_IDS[5]])
def test_pcg_resumes_bit_for_bit(idx, dtype_name):
	"""Ten calls of 5 iterations against one call of 50 (a padded row stride of Xt on one side): the same bits in X and in every output."""
	one = case_solver(idx, dtype_name).run(50).get()
	s = case_solver(idx, dtype_name, pad=5)
	for _ in range(10):
		s.run(5)
	ten = s.get()
	for k in ("X", "relres", "bx", "its"):
		assert np.array_equal(one[k], ten[k]), k
	assert np.all(one["its"] > 0) and np.all(one["its"] <= 50)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_pcg_frozen_and_zero_columns_do_not_move(dtype_name):
	"""se 300 without a preconditioner, right-hand sides (an eigenvector of A, y, 0): plain CG converges on an eigenvector in ONE iteration (the
	eigenvector is exact to eps x cond, far below tol), so column 0 is frozen after the first of 5 iterations, and the zero column from the
	start.  20 further iterations move y's column and leave the other two, and their counters, bit-unchanged."""
	idx = 3
	kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
	o = KO.oracle_run(idx, dtype_name)
	v = np.linalg.eigh(o["A64"])[1][:, -1]
	if dtype_name == "float32":
		v = v.astype(np.float32).astype(np.float64)
	B = np.stack([v, o["B64"][:, 0], np.zeros(n)], axis=1)
	s = Solver(kind, o["x"], gamma, B, dtype_name, o["s"] ** 2, tol=o["tol"]).run(5)
	a = s.get()
	b = s.run(20).get()
	assert a["its"][0] == 1 and a["relres"][0] <= o["tol"] and KO.true_relres(o["A64"], B, a["X"])[0] <= 2 * o["tol"]
	assert a["its"][2] == 0 and a["relres"][2] == 0 and a["bx"][2] == 0 and np.all(a["X"][:, 2] == 0)
	assert a["its"][1] == 5 and b["its"][1] == 25 and not np.array_equal(a["X"][:, 1], b["X"][:, 1])
	for c in (0, 2):
		assert np.array_equal(a["X"][:, c], b["X"][:, c]) and a["its"][c] == b["its"][c] and a["relres"][c] == b["relres"][c] and a["bx"][c] == b["bx"][c]


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("idx", [0, 4], ids=[KO.PCG_IDS[0], KO.PCG_IDS[4]])
def test_pcg_without_a_preconditioner(idx, dtype_name):
	"""r = 0 is plain CG: it solves as well, in more iterations than the preconditioned run, and in about the oracle's plain count."""
	o = KO.oracle_run(idx, dtype_name)
	got = case_solver(idx, dtype_name, precond=False).solve(block=10).get()
	true = KO.true_relres(o["A64"], o["B64"], got["X"])
	print("%s %s plain: %d iterations (oracle %d), true residual / tol %.3f" % (KO.PCG_IDS[idx], dtype_name, got["its"].max(), o["its_plain"].max(), true.max() / o["tol"]))
	assert np.all(true <= 2 * o["tol"])
	assert got["its"].max() > solved(idx, dtype_name)["its"].max()


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_pcg_flags_a_curvature_that_is_not_positive(dtype_name):
	"""Two far-apart points with diag_add = -10: the operator is -9 I up to exp(-800), <P, A P> is negative at the first iteration.  An ordinary
	arithmetic outcome: the column is flagged with its = -1, X stays at the last good iterate (0), nothing else happens."""
	x = np.array([[-1.0, 0.0], [1.0, 0.0]])
	B = np.array([[1.0, 0.0], [2.0, 0.0]])          # (the second column is zero: it is not flagged)
	got = Solver("se", x, 0.05, B, dtype_name, -10.0, tol=1e-6).run(7).get()
	assert got["its"][0] == -1 and got["its"][1] == 0
	assert np.all(np.isfinite(got["X"])) and np.all(got["X"] == 0)
	assert got["relres"][0] == 1 and got["bx"][0] == 0
