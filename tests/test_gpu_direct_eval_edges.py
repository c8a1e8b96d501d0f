"""
The direct-difference kernel evaluator on the device (pc_phi and the distance loops of csrc/pchol.hip and csrc/kmv.hip) on ARD, off-centre
and edge inputs, through everything that stands on it: stpy_kmv, stpy_pchol, stpy_pcg, IterativeGaussianProcess and
NystromFeatures(approx="pivoted").  The inputs are those of tests/direct_eval_cases.py (tests/test_direct_eval_cases_cpu.py shows on the
CPU that they separate a right evaluator from a wrong one); both dtypes throughout, float32 runs on float32-exact inputs.

What is pinned, and by what:
  values       |Y - K| <= 2 eps (d + 8) |kappa| entry by entry against the longdouble truth (stpy_kmv with Vt = I returns the matrix itself;
               the factor 2 is the one tests/test_gpu_kmv.py grants the hardware's exp), on ARD inverse lengthscales that are distinct in
               every coordinate -- a wrong lengthscale or column index moves values by orders of magnitude more;
  translation  every output on a layout's integer translate (its "twin") has the SAME BITS as on the centred layout: the coordinates are
               subtracted before they are scaled, the differences are exact, so nothing the evaluator computes sees the offset.  This is
               the primary check of the order of the two operations; the bound catches the other order too where the CPU file says so;
  exactness    kappa (+ diag_add) on every coincident pair, bitwise symmetry when a is b, kappa a pure scale (powers of two: same bits);
  pivoting     the replay checks of tests/test_gpu_pchol.py with a lengthscale vector; K = kappa I (the lattice) ties every residual at every
               step, so pivots 0, 1, 2, ... across several tiles pin "lowest index" over the whole grid and the double-buffered partials.
Each entry-level test prints its largest error / bound (`-s` shows them).
"""
import numpy as np
import pytest
import torch

from tests import direct_eval_cases as D
from tests import gram_edge_cases as E
from tests import kmv_oracle as KO
from tests import nystrom_oracle as NO

pytestmark = pytest.mark.gpu

KAPPA = 1.5
DTS = ["f64", "f32"]
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
DT_NAME = {"f64": "float64", "f32": "float32"}
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def L(gpu_device):
	from stpy_amd import _lib
	return _lib


@pytest.fixture(autouse=True)
def _drop_cached_cases():
	yield
	E.make_case.cache_clear()


def dev(v, dt):
	return torch.from_numpy(np.array(v, order="C")).to(device="cuda:0", dtype=TORCH_DT[dt])


def dev_cols(cols):
	return torch.tensor(list(cols), dtype=torch.int32, device="cuda:0") if cols is not None else None


def run_kmv(L, case, kind, V=None, kappa=KAPPA, diag_add=0.0, cols=None, inv_ls=None):
	"""Yt (t, n) of stpy_kmv on the case's points for V (q, t) (default: the identity, so that Yt[j][i] = k(a_i, b_j) + diag_add [i == j], laid out
	as the truth of gram_edge_cases); cols / inv_ls override the case's."""
	dt = case.dt
	ad = dev(case.a, dt)
	bd = ad if case.same else dev(case.b, dt)
	V = np.eye(case.q) if V is None else V
	Vt = dev(V.T, dt)
	Yt = torch.full((Vt.shape[0], case.n), float("nan"), dtype=ad.dtype, device=ad.device)
	L.kmv(kind, ad, bd, Vt, Yt, dev(case.inv_ls if inv_ls is None else inv_ls, dt), cols=dev_cols(cols), kappa=kappa, diag_add=diag_add)
	torch.cuda.synchronize()
	return Yt.cpu().numpy()


def value_bound(case, kappa=KAPPA):
	return 2.0 * E.direct_bound(case, kappa)


# ---------------------------------------------------------------------------------------------------------------- kernel values
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", D.DIMS)
def test_values_entry_by_entry(L, d, dt):
	"""Every layout of direct_eval_cases.entry_cases at n = q = 129 (a is b, diag_add = 0.25) and n = 70 against q = 150, all four kinds:
	within the bound of the truth, finite, bitwise symmetric, exactly kappa (+ diag_add) on coincident pairs, the same bits on a twin.
	One grid step apart (float64, 2^-30): below kappa wherever the rounded truth is -- Matern 1/2; the truth of Matern 3/2 and 5/2,
	1 - 4e-19, rounds to 1 -- and never above kappa."""
	T = E.DTYPES[dt]
	worst = {}
	for (n, q, same) in D.SHAPES:
		diag_add = 0.25 if same else 0.0
		got_of = {}
		for name, case, base in D.entry_cases(d, dt, n, q, same):
			r2, _, _ = E.sq_dist_and_dot(case)
			coincident = r2 == 0
			bound = value_bound(case)
			extra = diag_add * np.eye(n) if same else 0.0
			for kind in D.KINDS:
				Y = run_kmv(L, case, kind, diag_add=diag_add)
				got_of[(name, kind)] = Y
				assert Y.dtype == T and Y.shape == (q, n)
				assert np.all(np.isfinite(Y)), (name, kind)
				t = E.truth_ld(case, kind, KAPPA) + extra
				ratio = float(np.max(np.abs(Y.astype(E.LD) - t)) / bound)
				worst[name] = max(worst.get(name, 0.0), ratio)
				assert ratio <= 1.0, (name, kind, same, ratio)
				if same:
					assert np.array_equal(Y, Y.T), (name, kind)
					assert np.all(np.diag(Y) == T(KAPPA + diag_add)), (name, kind)
					off = coincident & ~np.eye(n, dtype=bool)
				else:
					off = coincident
				assert np.all(Y[off] == T(KAPPA)), (name, kind)
				if name.startswith("duplicates"):
					assert int(off.sum()) >= (2 if same else 1) * E.N_DUP          # (the float32 grid at d = 1 adds chance coincidences)
					if dt == "f64" and kind != E.SE:
						near = (r2 > 0) & (r2 < 1e-15)
						assert int(near.sum()) == (2 if same else 1) * E.N_NEAR
						below = E.truth(case, kind, KAPPA)[near] < KAPPA
						assert np.all(Y[near][below] < KAPPA) and np.all(Y[near] <= KAPPA), (name, kind)
						assert np.all(below) == (kind == E.M12)
				if base is not None:
					assert np.array_equal(Y, got_of[(base, kind)]), "%s %s: the twin does not have the bits of %s" % (name, D.KIND_NAME[kind], base)
	for name in sorted(worst):
		print("DIRECTEDGE values %s d=%-2d %-28s largest error / bound %.3g" % (dt, d, name, worst[name]))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", (12, 20, 33))
def test_values_through_a_column_subset(L, d, dt):
	"""d coordinates read as a shuffled subset of a 40-wide x (the 16-coordinate register form and two and three rounds through LDS) with the
	ARD vector: bit-equal to the run on the gathered columns, and within the bound of the truth."""
	worst = 0.0
	for (n, q, same) in D.SHAPES:
		wide, cols, g = D.wide_case("cube", d, dt, n, q, same)
		for kind in D.KINDS:
			Yw = run_kmv(L, wide, kind, cols=cols, inv_ls=g.inv_ls)
			Yg = run_kmv(L, g, kind)
			assert np.array_equal(Yw, Yg), (kind, same)
			ratio = float(np.max(np.abs(Yw.astype(E.LD) - E.truth_ld(g, kind, KAPPA))) / value_bound(g))
			worst = max(worst, ratio)
			assert ratio <= 1.0, (kind, same, ratio)
	print("DIRECTEDGE cols %s d=%-2d largest error / bound %.3g" % (dt, d, worst))


@pytest.mark.parametrize("dt", DTS)
def test_kappa_is_a_pure_scale(L, dt):
	"""kappa = 4 with diag_add = 4 c against kappa = 1 with diag_add = c (c = 0.25): four times the same bits.  kappa = -0.75 within the bound."""
	for d in (3, 20):
		case = D.ard_case("cube", d, dt, 129, 129, True)
		for kind in D.KINDS:
			one = run_kmv(L, case, kind, kappa=1.0, diag_add=0.25)
			four = run_kmv(L, case, kind, kappa=4.0, diag_add=1.0)
			assert np.array_equal(four, 4 * one), (d, kind)
			neg = run_kmv(L, case, kind, kappa=-0.75)
			ratio = float(np.max(np.abs(neg.astype(E.LD) - E.truth_ld(case, kind, -0.75))) / value_bound(case, -0.75))
			print("DIRECTEDGE kappa=-0.75 %s d=%-2d %-8s largest error / bound %.3g" % (dt, d, D.KIND_NAME[kind], ratio))
			assert ratio <= 1.0 and np.all(neg <= 0) and np.all(np.diag(neg) == -0.75)


# ---------------------------------------------------------------------------------------------------------------- products
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("t", (3, 17))
@pytest.mark.parametrize("d", (3, 20))
def test_kmv_products_on_ard_and_off_centre_points(L, d, t, dt):
	"""A real V: per entry 2 eps (q + d + 8) (|K| |V|), the bound of tests/test_gpu_kmv.py, with K the longdouble truth.  n = 5 against q = 1300
	has its j range cut into 6 pieces (kp_split), n = q = 129 (a is b, diag_add = 0.1) runs uncut.  Each twin gives the same bits."""
	T = E.DTYPES[dt]
	worst = 0.0
	for (n, q, same) in ((5, 1300, False), (129, 129, True)):
		case = D.ard_case("cube", d, dt, n, q, same)
		V = np.random.RandomState(8800 + d + t).standard_normal((q, t)).astype(T).astype(np.float64)
		diag_add = 0.1 if same else 0.0
		for kind in D.KINDS:
			Yt = run_kmv(L, case, kind, V=V, diag_add=diag_add)
			K = E.truth(case, kind, KAPPA)                                  # (q, n)
			ref, mag = K.T @ V, np.abs(K).T @ np.abs(V)
			if same:
				ref, mag = ref + diag_add * V, mag + diag_add * np.abs(V)
			bound = 2 * case.eps * (q + d + 8) * mag
			err = np.abs(Yt.T.astype(np.float64) - ref)
			worst = max(worst, float((err / bound).max()))
			assert np.all(np.isfinite(Yt)) and np.all(err <= bound), (kind, same, float((err / bound).max()))
			for shift in ("offset", "offset_per_column"):
				assert np.array_equal(run_kmv(L, D.twin(case, shift), kind, V=V, diag_add=diag_add), Yt), (kind, same, shift)
	print("DIRECTEDGE product %s d=%-2d t=%-2d largest error / bound %.3g" % (dt, d, t, worst))


# ---------------------------------------------------------------------------------------------------------------- pivoted Cholesky
def run_pchol(L, x, dt, kind, inv_ls, m, cols=None, kappa=1.0, tol=0.0):
	piv, Ft, dres, rank = L.pchol(kind, dev(x, dt), dev(inv_ls, dt), m, cols=dev_cols(cols), kappa=kappa, tol=tol)
	torch.cuda.synchronize()
	return piv.cpu().numpy(), Ft.cpu().numpy(), dres.cpu().numpy(), int(rank.item())


PCHOL_N, PCHOL_M = 777, 33
# (kind, d, through a column subset of a 40-wide x, the twin's shift)
PCHOL_CASES = [(E.SE, 3, False, "offset"), (E.M52, 3, False, "offset"), (E.SE, 20, True, "offset_per_column"), (E.M52, 20, True, "offset_per_column")]
PCHOL_IDS = ["%s-d%d%s" % (D.KIND_NAME[c[0]], c[1], "-cols" if c[2] else "") for c in PCHOL_CASES]


def pchol_inputs(idx, dt):
	"""(the case that holds x, cols or None, the case of the coordinates read, the twin of the first)."""
	kind, d, wide, shift = PCHOL_CASES[idx]
	if wide:
		w, cols, g = D.wide_case("cube", d, dt, PCHOL_N, PCHOL_N, True)
	else:
		w = g = D.ard_case("cube", d, dt, PCHOL_N, PCHOL_N, True)
		cols = None
	return w, cols, g, D.twin(w, shift)


def replay(kind, x, gamma, m, cols, pv, dt, kappa=1.0):
	"""The float64 oracle with the device's pivots forced (and the float32 one for the float32 tolerance): the rule of tests/test_gpu_pchol.py."""
	tr = []
	_, F64, d64, _ = NO.pivoted_cholesky(D.KIND_NAME[kind], x, gamma, m, kappa=kappa, cols=cols, pivots=pv, trace=tr)
	out = dict(F64=F64, d64=d64, trace=tr, tol=1e-8)
	if dt == "f32":
		_, F32, d32, _ = NO.pivoted_cholesky(D.KIND_NAME[kind], x.astype(np.float32), gamma, m, kappa=kappa, cols=cols, pivots=pv, dtype=np.float32)
		own = max(np.abs(F32 - F64).max(), np.abs(d32 - d64).max())
		out.update(own=own, tol=max(8.0 * own, 16.0 * EPS32))
	return out


def replay_checks(tag, got, rep, n, m):
	"""Validity, factor and greediness at every step; ``got`` = (piv, Ft, dres, rank) of the device, ``rep`` = replay(...) of its pivots."""
	piv, Ft, dres, rank = got
	assert rank == m
	assert piv.min() >= 0 and piv.max() < n and len(set(piv.tolist())) == m and piv[0] == 0
	assert np.all(np.isfinite(Ft)) and np.all(np.isfinite(dres)) and np.all(dres[piv] == 0)
	eF, ed = np.abs(Ft - rep["F64"]).max(), np.abs(dres - rep["d64"]).max()
	shortfall = max(top - at for at, top in rep["trace"])
	print("DIRECTEDGE pchol %s: |Ft - replay| %.3e  |dres - replay| %.3e  largest shortfall of a pivot %.3e  tolerance %.3e" % (tag, eF, ed, shortfall, rep["tol"]))
	assert eF <= rep["tol"] and ed <= rep["tol"]
	assert len(rep["trace"]) == m
	for j, (at, top) in enumerate(rep["trace"]):
		assert at >= top - rep["tol"], (j, at, top)


_PCHOL = {}


def pchol_result(L, idx, dt):
	"""One device run (kappa = 1, tol = 0) and its replay per case and dtype, shared by the tests."""
	if (idx, dt) not in _PCHOL:
		kind = PCHOL_CASES[idx][0]
		w, cols, g, tw = pchol_inputs(idx, dt)
		got = run_pchol(L, w.a, dt, kind, g.inv_ls, PCHOL_M, cols)
		ok = got[3] == PCHOL_M and got[0].min() >= 0 and got[0].max() < PCHOL_N and len(set(got[0].tolist())) == PCHOL_M
		_PCHOL[(idx, dt)] = dict(got=got, rep=replay(kind, w.a, D.gamma_of(g), PCHOL_M, cols, got[0], dt) if ok else None)
	return _PCHOL[(idx, dt)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("idx", range(len(PCHOL_CASES)), ids=PCHOL_IDS)
def test_pchol_replay_on_ard_points(L, idx, dt):
	r = pchol_result(L, idx, dt)
	assert r["rep"] is not None, "rank %d, pivots %s" % (r["got"][3], r["got"][0])
	replay_checks("%s %s" % (PCHOL_IDS[idx], dt), r["got"], r["rep"], PCHOL_N, PCHOL_M)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("idx", range(len(PCHOL_CASES)), ids=PCHOL_IDS)
def test_pchol_twin_has_the_same_bits(L, idx, dt):
	kind = PCHOL_CASES[idx][0]
	w, cols, g, tw = pchol_inputs(idx, dt)
	got = pchol_result(L, idx, dt)["got"]
	moved = run_pchol(L, tw.a, dt, kind, g.inv_ls, PCHOL_M, cols)
	for name, u, v in zip(("piv", "Ft", "dres"), got, moved):
		assert np.array_equal(u, v), name
	assert got[3] == moved[3]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("idx", range(len(PCHOL_CASES)), ids=PCHOL_IDS)
def test_pchol_kappa_is_a_pure_scale(L, idx, dt):
	"""kappa = 4 against kappa = 1 at the same tol: same pivots and rank, Ft exactly doubled, dres exactly quadrupled -- at tol = 0 (rank m) and
	at a tol that stops the run early.  That tol is the geometric mean of the pivot residual of a step of the replay and the smallest
	one before it, at the step where it is furthest from both; the device's residuals are within the replay tolerance of the replay's, so the stop is decided where both neighbours are
	further than 4 x that tolerance from tol * kappa (asserted).  The later one lies above tol / 4 (asserted): a threshold that forgot kappa
	would not stop there at kappa = 4."""
	kind = PCHOL_CASES[idx][0]
	w, cols, g, tw = pchol_inputs(idx, dt)
	r = pchol_result(L, idx, dt)
	assert r["rep"] is not None
	at = np.array([a for a, _ in r["rep"]["trace"]])

	def margin(j):
		tj = np.sqrt(at[:j].min() * at[j])
		return min(at[:j].min() - tj, tj - at[j], at[j] - tj / 4)
	j = max(range(2, PCHOL_M), key=margin)
	tol = float(np.sqrt(at[:j].min() * at[j]))
	print("DIRECTEDGE pchol %s %s: stop expected at step %d, pivot residuals %.3e > tol %.3e > %.3e" % (PCHOL_IDS[idx], dt, j, at[:j].min(), tol, at[j]))
	assert at[:j].min() - tol >= 4 * r["rep"]["tol"] and tol - at[j] >= 4 * r["rep"]["tol"] and at[j] > tol / 4 + 4 * r["rep"]["tol"]
	for tl, rank in ((0.0, PCHOL_M), (tol, j)):
		one = r["got"] if tl == 0.0 else run_pchol(L, w.a, dt, kind, g.inv_ls, PCHOL_M, cols, kappa=1.0, tol=tl)
		four = run_pchol(L, w.a, dt, kind, g.inv_ls, PCHOL_M, cols, kappa=4.0, tol=tl)
		assert one[3] == rank and four[3] == rank
		assert np.array_equal(one[0], four[0]) and np.all(one[0][rank:] == -1)
		assert np.array_equal(four[1], 2 * one[1]) and np.array_equal(four[2], 4 * one[2])
		assert np.all(one[1][rank:] == 0) and np.array_equal(one[0][:rank], r["got"][0][:rank])


@pytest.mark.parametrize("dt", DTS)
def test_pchol_lattice_breaks_ties_across_tiles(L, dt):
	"""K = 4 I on 600 points (5 tiles in float64, 3 in float32), m = 300: every residual ties at every step.  Pivots 0 .. 299 in order, Ft and
	dres exactly the oracle's (Ft[j] = 2 e_j; dres 0 on the pivots, 4 elsewhere), rank 300, for all four kinds."""
	c = D.lattice_case(dt)
	T = c.np_dtype
	m = D.LATTICE_M
	for kind in D.KINDS:
		piv_o, Ft_o, dres_o, rank_o = NO.pivoted_cholesky(D.KIND_NAME[kind], c.a.astype(T), D.gamma_of(c), m, kappa=D.LATTICE_KAPPA, dtype=T)
		piv, Ft, dres, rank = run_pchol(L, c.a, dt, kind, c.inv_ls, m, kappa=D.LATTICE_KAPPA)
		assert rank == m == rank_o
		assert np.array_equal(piv, np.arange(m)) and np.array_equal(piv_o, np.arange(m)), (kind, piv[:8])
		assert np.array_equal(Ft, Ft_o) and np.array_equal(dres, dres_o), kind
		assert np.all(Ft[np.arange(m), np.arange(m)] == 2) and np.count_nonzero(Ft) == m
		assert np.all(dres[:m] == 0) and np.all(dres[m:] == 4)


@pytest.mark.parametrize("dt", DTS)
def test_pchol_nearly_flat_stops_at_rank_one(L, dt):
	"""inv_ls = 2^-20: the residual after the first step is 2e-11 (float64) / 2.4e-7 (float32) on the oracle, two orders and more below tol."""
	c = D.flat_case(dt)
	tol = D.FLAT_TOL[dt]
	for kind in D.FLAT_KINDS:
		piv, Ft, dres, rank = run_pchol(L, c.a, dt, kind, c.inv_ls, 8, tol=tol)
		assert rank == 1 and piv[0] == 0 and np.all(piv[1:] == -1), (kind, rank, piv)
		assert np.all(Ft[1:] == 0) and np.all(np.isfinite(Ft[0]))
		assert np.abs(dres).max() <= tol and dres[piv[0]] == 0


@pytest.mark.parametrize("dt", DTS)
def test_pchol_tiny_lengthscale(L, dt):
	"""inv_ls = 64 at d = 3: K is the identity up to a few entries, among them denormals of the dtype.  Rank m, finite outputs, the replay checks."""
	c = E.make_case("tiny_lengthscale", 3, dt, PCHOL_N, PCHOL_N, True)
	for kind in D.KINDS:
		got = run_pchol(L, c.a, dt, kind, c.inv_ls, PCHOL_M)
		assert got[3] == PCHOL_M and len(set(got[0].tolist())) == PCHOL_M and got[0].min() >= 0 and got[0].max() < PCHOL_N
		replay_checks("tiny_lengthscale %s %s" % (D.KIND_NAME[kind], dt), got, replay(kind, c.a, D.gamma_of(c), PCHOL_M, None, got[0], dt), PCHOL_N, PCHOL_M)


# ---------------------------------------------------------------------------------------------------------------- block PCG
PCG_KIND, PCG_KAPPA, PCG_RANK = E.M32, 2.5, 33


def pcg_solve(L, x, dt, inv_ls, B, G, s, tol, block=10, maxiter=3000):
	"""stpy_pcg on (kappa K(x, x) + s^2 I) X = B in blocks of ``block`` iterations until every column has stopped."""
	tdt = TORCH_DT[dt]
	xd, ild = dev(x, dt), dev(inv_ls, dt)
	n, t = B.shape
	Bt = dev(B.T, dt)
	Xt = torch.full((t, n), float("nan"), dtype=tdt, device="cuda:0")
	Gn = dev(G, dt)
	Gt = Gn.t().contiguous()
	work = L.pcg_workspace(n, x.shape[1], t, G.shape[1], xd)
	out = (torch.empty(t, dtype=tdt, device="cuda:0"), torch.empty(t, dtype=tdt, device="cuda:0"), torch.empty(t, dtype=torch.int32, device="cuda:0"))
	done = 0
	while done < maxiter:
		L.pcg(PCG_KIND, xd, ild, Bt, Xt, work, out, kappa=PCG_KAPPA, diag_add=s * s, Gt=Gt, Gn=Gn, tol=tol, iters=block, init=done == 0)
		done += block
		rel, its = out[0].cpu().numpy(), out[2].cpu().numpy()
		if np.all((rel <= tol) | (its < 0)):
			break
	return dict(X=Xt.cpu().numpy().T.copy(), relres=out[0].cpu().numpy(), bx=out[1].cpu().numpy(), its=out[2].cpu().numpy())


@pytest.mark.parametrize("dt", DTS)
def test_pcg_on_an_ard_problem_and_its_twin(L, dt):
	"""n = 777, d = 3, Matern 3/2, kappa = 2.5, the oracle's rank-33 preconditioner in the working dtype, right-hand sides y and five kernel
	columns; s and tol of kmv_oracle.SETTINGS.  Recurrence residual <= tol, true float64 residual <= 2 tol, iterations at most the
	geometric mean of the oracle's preconditioned and plain counts (where their ratio is below 0.5), as in tests/test_gpu_pcg.py.  The
	solve on the translated points gives the same bits in every output."""
	T = E.DTYPES[dt]
	s, tol = KO.SETTINGS[DT_NAME[dt]]
	case = D.ard_case("cube", 3, dt, PCHOL_N, PCHOL_N, True)
	x, gamma, n = case.a, D.gamma_of(case), case.n
	kname = D.KIND_NAME[PCG_KIND]
	rng = np.random.RandomState(8900)
	y = (np.sin(3.0 * x @ rng.uniform(-1, 1, size=3)) + 0.1 * rng.standard_normal(n)).astype(T).astype(np.float64)
	xt = rng.uniform(-1, 1, size=(5, 3)).astype(T).astype(np.float64)
	B = np.concatenate([y.reshape(-1, 1), NO.kernel(kname, x, xt, gamma, PCG_KAPPA)], axis=1).astype(T).astype(np.float64)
	A64 = NO.kernel(kname, x, x, gamma, PCG_KAPPA) + s * s * np.eye(n)
	A = (NO.kernel(kname, x, x, gamma, PCG_KAPPA, dtype=T) + T(s * s) * np.eye(n, dtype=T)).astype(T)
	G = KO.preconditioner(kname, x, gamma, s, PCG_RANK, dtype=T, kappa=PCG_KAPPA)
	assert G.shape == (n, PCG_RANK)
	_, its_pre, _ = KO.pcg(A, B, tol, 5000, G=G, dtype=T)
	_, its_plain, _ = KO.pcg(A, B, tol, 5000, G=None, dtype=T)
	got = pcg_solve(L, x, dt, case.inv_ls, B, G, s, tol)
	true = KO.true_relres(A64, B, got["X"])
	its, pre, plain = int(got["its"].max()), int(its_pre.max()), int(its_plain.max())
	print("DIRECTEDGE pcg %s: true residual / tol %.3f, recurrence %.3f; iterations %d (oracle %d preconditioned, %d plain, geometric mean %.1f)" % (
		dt, true.max() / tol, got["relres"].max() / tol, its, pre, plain, np.sqrt(pre * plain)))
	assert np.all(np.isfinite(got["X"])) and np.all(got["its"] > 0)
	assert np.all(got["relres"] <= tol)
	assert np.all(true <= 2 * tol)
	if pre / plain < 0.5:
		assert its <= np.sqrt(pre * plain)
	moved = pcg_solve(L, D.twin(case, "offset").a, dt, case.inv_ls, B, G, s, tol)
	for k in ("X", "relres", "bx", "its"):
		assert np.array_equal(got[k], moved[k]), k


# ---------------------------------------------------------------------------------------------------------------- the classes
GP_M = 37


def ard_kernel_object(name, gamma, kappa=1.0, d=None, group=None):
	from stpy_amd import KernelFunction
	kw = dict(ard_gamma=torch.from_numpy(np.array(gamma)), kappa=kappa, d=len(gamma) if d is None else d, group=group)
	return KernelFunction(kernel_name="ard", **kw) if name == "ard" else KernelFunction(kernel_name="ard_matern", nu=1.5, **kw)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ("ard", "ard_matern"))
def test_iterative_gp_with_an_ard_kernel(L, name, dt):
	"""IterativeGaussianProcess with unequal lengthscales (d = 3, n = 777, 37 test points, kappa = 1.3): mean and variance within
	kmv_oracle.posterior_bounds evaluated with the lengthscale vector; float64 also against GaussianProcess with the same kernel, within
	those bounds plus 1e-8, as tests/test_gpu_iterative_gp.py does; the fit on the translated data and test points gives a bit-equal mean."""
	from stpy_amd import GaussianProcess, IterativeGaussianProcess
	T, tdt = E.DTYPES[dt], TORCH_DT[dt]
	s, tol = KO.SETTINGS[DT_NAME[dt]]
	kappa = 1.3
	case = D.ard_case("cube", 3, dt, PCHOL_N, GP_M)
	x, xt, gamma = case.a, case.b, D.gamma_of(case)
	rng = np.random.RandomState(9000)
	y = (np.sin(3.0 * x @ rng.uniform(-1, 1, size=3)) + 0.1 * rng.standard_normal(case.n)).astype(T).astype(np.float64).reshape(-1, 1)
	kind = "se" if name == "ard" else "matern32"

	def fit(xs, xts):
		gp = IterativeGaussianProcess(kernel=ard_kernel_object(name, gamma, kappa), s=s, precond_rank=PCG_RANK, rhs_block=16)
		gp.fit_gp(torch.from_numpy(xs).to(tdt), torch.from_numpy(y).to(tdt))
		return gp
	gp = fit(x, xt)
	mu, std = gp.mean_std(torch.from_numpy(xt).to(tdt))
	mu, var = mu.numpy().astype(np.float64), std.numpy().astype(np.float64) ** 2
	mu_o, var_o, b_mu, b_var = KO.posterior_bounds(kind, x, y, xt, gamma, s, tol, KO.eps_of(T), None, kappa)
	e_mu, e_var = np.abs(mu - mu_o), np.abs(var - var_o)
	print("DIRECTEDGE gp %s %s: mean error / bound %.3g, variance error / bound %.3g, fit: %s" % (name, dt, (e_mu / b_mu).max(), (e_var / b_var).max(), gp.cg_info))
	assert mu.shape == (GP_M, 1) and np.all(np.isfinite(mu)) and np.all(np.isfinite(var))
	assert gp.cg_info["rank"] == PCG_RANK
	assert np.all(e_mu <= b_mu)
	assert np.all(e_var <= b_var)
	if dt == "f64":
		exact = GaussianProcess(kernel=ard_kernel_object(name, gamma, kappa), s=s)
		exact.fit_gp(torch.from_numpy(x), torch.from_numpy(y))
		mu_e, std_e = exact.mean_std(torch.from_numpy(xt))
		assert np.all(np.abs(mu - mu_e.numpy()) <= b_mu + 1e-8)
		assert np.all(np.abs(var - std_e.numpy() ** 2) <= b_var + 1e-8)
	tw = D.twin(case, "offset")
	moved = fit(tw.a, tw.b)
	assert np.array_equal(moved.mean(torch.from_numpy(tw.b).to(tdt)).numpy(), gp.mean(torch.from_numpy(xt).to(tdt)).numpy())
	assert np.array_equal(moved.A.numpy(), gp.A.numpy())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("idx", (0, 2), ids=[PCHOL_IDS[0], PCHOL_IDS[2]])
def test_nystrom_pivoted_with_an_ard_kernel(L, idx, dt):
	"""NystromFeatures(approx="pivoted") on an `ard` kernel object -- at d = 3, and at d = 20 as a `group` of a 40-wide x, where the class has to
	pair ard_gamma[group[k]] with column group[k]: its landmarks are the pivots of the direct _lib.pchol call with that inv_ls, and
	trace_error matches the replay by the rule of tests/test_gpu_pchol.py (tolerance times n)."""
	from stpy_amd import NystromFeatures
	w, cols, g, tw = pchol_inputs(idx, dt)
	r = pchol_result(L, idx, dt)
	assert r["rep"] is not None
	gamma = D.gamma_of(g)
	if cols is None:
		kernel = ard_kernel_object("ard", gamma)
	else:
		wide_gamma = np.ones(w.a.shape[1])
		wide_gamma[cols] = gamma
		kernel = ard_kernel_object("ard", wide_gamma, d=w.a.shape[1], group=list(cols))
	x = torch.from_numpy(w.a).to(TORCH_DT[dt])
	nys = NystromFeatures(kernel, m=PCHOL_M, approx="pivoted", s=0.1)
	nys.fit_gp(x, torch.zeros(PCHOL_N, 1, dtype=x.dtype))
	assert np.array_equal(np.asarray(nys.C), r["got"][0])
	want = PCHOL_N * 1.0 - float(np.sum(r["rep"]["F64"] * r["rep"]["F64"]))
	got = float(nys.trace_error)
	print("DIRECTEDGE nystrom %s %s: trace_error %.10e, replay %.10e, tolerance %.3e" % (PCHOL_IDS[idx], dt, got, want, r["rep"]["tol"] * PCHOL_N))
	assert abs(got - want) <= r["rep"]["tol"] * PCHOL_N
