"""
Gram kernels through the C ABI on off-centre, duplicate and extreme-scale inputs (tests/gram_edge_cases.py has the inputs, the
longdouble truth and the derived bounds).  Every assertion is element-wise max-abs against a bound: the faults these tests look for
sit on a few entries (the diagonal, duplicates), which a norm ratio averages away.  Each case prints its measured error and bound
(`-s` shows them; DESIGN.md "Gram accuracy off the unit cube" tabulates them).  Run with `-m gpu` on an MI355X.
"""
import numpy as np
import pytest
import torch

from tests import gram_edge_cases as E

pytestmark = pytest.mark.gpu

KAPPA = 1.3
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
# (name, kind as the truth knows it, degree, offset)
VARIANTS = [("se", E.SE, 0, 0.0), ("m12", E.M12, 0, 0.0), ("m32", E.M32, 0, 0.0), ("m52", E.M52, 0, 0.0), ("lin", E.LIN, 0, 0.25)] + \
           [("poly%d" % p, E.POLY, p, 1.0) for p in E.POLY_DEGREES]


@pytest.fixture(scope="module")
def L(gpu_device):
	from stpy_amd import _lib
	return _lib


@pytest.fixture(autouse=True)
def _drop_cached_cases():
	yield
	E.make_case.cache_clear()


def dev(a, dt):
	return torch.from_numpy(np.array(a, order="C")).to(device="cuda:0", dtype=TORCH_DT[dt])


def abi_kind(kind, degree):
	return kind | (degree << 8)


def workspace(L, n, q, d, dt):
	nbytes = int(L.load().stpy_gram_workspace_bytes(L.dtype_code(TORCH_DT[dt]), n, q, d))
	return torch.empty((max(nbytes, 16),), dtype=torch.uint8, device="cuda:0")


def run_gram(L, case, kind, degree, use_ws, kappa=KAPPA, offset=0.0, diag_add=0.0, lower_only=0, combine=0, out=None, ldo=None, cols=None, inv_ls=None,
             d=None):
	"""stpy_gram on the case's points; returns the (q, ldo) output as float64 numpy.  cols / inv_ls / d override the case's."""
	dt = case.dt
	lib = L.load()
	ad = dev(case.a, dt)
	bd = ad if case.same else dev(case.b, dt)
	ild = dev(case.inv_ls if inv_ls is None else inv_ls, dt)
	d = case.d if d is None else d
	cd = torch.tensor(list(cols), dtype=torch.int32, device="cuda:0") if cols is not None else None
	ldo = case.n if ldo is None else ldo
	if out is None:
		out = torch.full((case.q, ldo), -7.0, dtype=TORCH_DT[dt], device="cuda:0")
	ws = workspace(L, case.n, case.q, d, dt) if use_ws else None
	L.check(lib.stpy_gram(abi_kind(kind, degree), L.dtype_code(TORCH_DT[dt]), L.ptr(ad), case.n, case.a.shape[1], L.ptr(bd), case.q, case.b.shape[1], d,
	                      L.ptr(cd), L.ptr(ild), kappa, offset, diag_add, lower_only, combine, L.ptr(out), ldo,
	                      L.ptr(ws), ws.numel() if ws is not None else 0, L.stream_ptr()), "gram")
	return out.cpu().numpy().astype(np.float64)


def tolerance(case, kind, degree, offset, use_ws, kappa=KAPPA):
	"""Scalar or (q, n) bound of the route that serves (kind, workspace)."""
	if kind in E.STATIONARY:
		return E.stationary_bound(case, kind, use_ws, kappa)
	return E.dot_kind_bound(case, kind, kappa, offset, degree)


def check_values(got, case, name, kind, degree, offset, use_ws, route, mask=None, extra=None, kappa=KAPPA):
	"""Element-wise comparison with the truth; returns a failure string or None, and prints the figures."""
	t = E.truth_ld(case, kind, kappa, offset, degree)
	if extra is not None:
		t = t + extra
	tol = tolerance(case, kind, degree, offset, use_ws, kappa)
	fmax = E.LD(np.finfo(case.np_dtype).max)
	with np.errstate(invalid="ignore", over="ignore"):
		representable = np.abs(t) + tol < fmax            # (POLY at an offset overflows the dtype: there the kernel owes +-inf or a huge value, not NaN)
		sel = representable if mask is None else (representable & mask)
		err = np.abs(got.astype(E.LD) - t)
		ratio = np.where(sel, err / tol, 0)
	bad_nan = np.isnan(got) if mask is None else (np.isnan(got) & mask)
	worst = float(np.max(ratio)) if ratio.size else 0.0
	e_abs = float(np.max(np.where(sel, err, 0)))
	tol_s = float(np.max(tol)) if np.ndim(tol) else float(tol)
	print("GRAMEDGE %-6s %s %-18s %-6s d=%-2d same=%d  max_abs_err %.3e  bound(max) %.3e  err/bound %.3g" % (
		name, case.dt, case.layout, route, case.d, case.same, e_abs, tol_s, worst))
	if bad_nan.any():
		return "%s %s d=%d: %d NaN entries" % (name, route, case.d, int(bad_nan.sum()))
	if not (stationary_finite(got, mask) if kind in E.STATIONARY else True):
		return "%s %s d=%d: non-finite entries" % (name, route, case.d)
	if worst > 1.0:
		return "%s %s d=%d same=%d: max_abs_err %.3e is %.3g x the bound" % (name, route, case.d, case.same, e_abs, worst)
	return None


def stationary_finite(got, mask):
	return bool(np.all(np.isfinite(got if mask is None else got[mask])))


def extreme_checks(got, case, name, kind, mask, kappa=KAPPA):
	"""tiny_lengthscale: entries >= 0 (SE may overshoot kappa, never go negative), at most 8 eps kappa where the truth has underflowed,
	exactly 0 or a denormal where the truth is below the smallest denormal; huge_lengthscale: within the bound of kappa, up to the
	distance of the truth itself from kappa."""
	sel = got if mask is None else got[mask]
	t = E.truth_ld(case, kind, kappa)
	t = t if mask is None else t[mask]
	fi = np.finfo(case.np_dtype)
	if case.layout == "tiny_lengthscale":
		if not np.all(sel >= 0):
			return "%s d=%d: negative entries" % (name, case.d)
		under = t < E.LD(fi.tiny)
		if np.any(sel[under] > 8 * case.eps * kappa):
			return "%s d=%d: %.3e where the truth has underflowed" % (name, case.d, float(sel[under].max()))
		gone = t < E.LD(fi.tiny) * E.LD(fi.eps) / 2
		if np.any(sel[gone] >= float(fi.tiny)):
			return "%s d=%d: a normal number (%.3e) where the truth is below the smallest denormal" % (name, case.d, float(sel[gone].max()))
	if case.layout == "huge_lengthscale":
		away = float(np.max(np.abs(t - E.LD(kappa))))
		if np.max(np.abs(sel - kappa)) > E.stationary_bound(case, kind, True, kappa) + away:
			return "%s d=%d: %.3e away from kappa" % (name, case.d, float(np.max(np.abs(sel - kappa))))
	return None


# ------------------------------------------------------------------------------------------------------------------------------
ROUTE_SHAPES = {"tile": ((300, 131, False), (200, 200, True)), "mfma": ((257, 513, False), (333, 333, True)), "fill": ((384, 640, False), (384, 384, True))}


@pytest.mark.parametrize("route", ["tile", "mfma", "fill"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("layout", E.LAYOUTS)
def test_gram_layouts_on_every_route(L, layout, dt, route):
	"""All six kinds (POLY at its five degrees) x every d, on one layout, dtype and route, against the truth at the bound of the route.
	tile: no workspace (the tile kernel; Matern by direct differences).  mfma: workspace and ragged shapes (prep + MFMA contraction with
	the fused epilogue; Matern 1/2 and POLY stay on the tile kernel).  fill: workspace and aligned overwriting shapes with route key 28
	at 1 and at 0 (fp64: the dedicated fill kernel against the aligned epilogue; fp32 has the aligned epilogue only), rectangular with a
	padded leading dimension whose padding must survive, and square lower-only with a == b (the `same` shortcut) and a diagonal term."""
	lib = L.load()
	failures = []
	keys = (1, 0) if (route == "fill" and dt == "f64") else (None,)
	assert lib.stpy_tune_get(28) == 1
	try:
		for key in keys:
			if key is not None:
				lib.stpy_tune(28, key)
			rname = route if key is None else "%s%d" % (route, key)
			for d in E.DIMS:
				for (n, q, same) in ROUTE_SHAPES[route]:
					case = E.make_case(layout, d, dt, n, q, same)
					use_ws = route != "tile"
					for (name, kind, degree, offset) in VARIANTS:
						mask = None
						if same and route == "fill":
							got = run_gram(L, case, kind, degree, use_ws, offset=offset, diag_add=0.37, lower_only=1)
							tiles = np.arange(q)[:, None] // 128 >= np.arange(n)[None, :] // 128
							if kind in (E.SE, E.M32, E.M52, E.LIN):          # the kinds whose lower-only fill works by 128 x 128 tiles
								if not np.all(got[~tiles] == -7.0):
									failures.append("%s %s d=%d: tiles above the diagonal were written" % (name, rname, d))
							mask = np.tril(np.ones((q, n), dtype=bool))
							f = check_values(got, case, name, kind, degree, offset, use_ws, rname, mask=mask, extra=E.LD(0.37) * np.eye(q, dtype=E.LD))
						elif route == "fill":
							got = run_gram(L, case, kind, degree, use_ws, offset=offset, ldo=n + 2)
							if not np.all(got[:, n:] == -7.0):
								failures.append("%s %s d=%d: padding of the leading dimension overwritten" % (name, rname, d))
							got = got[:, :n]
							f = check_values(got, case, name, kind, degree, offset, use_ws, rname)
						else:
							got = run_gram(L, case, kind, degree, use_ws, offset=offset)
							f = check_values(got, case, name, kind, degree, offset, use_ws, rname)
						if f:
							failures.append(f)
						if kind in E.STATIONARY and not (same and route == "fill"):
							f = extreme_checks(got, case, name, kind, mask)
							if f:
								failures.append(rname + " " + f)
	finally:
		lib.stpy_tune(28, 1)
	assert not failures, "\n".join(failures)


@pytest.mark.parametrize("use_ws", [False, True])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("layout", ["cube", "offset"])
def test_gram_options_cols_diag_ldo_combine(L, layout, dt, use_ws):
	"""A `cols` subset with its own inverse lengthscales, diag_add, a padded ldo, and combine ADD / MUL onto a previous kernel: the
	second term's error bound, plus the first term's propagated through the sum / product (|K2| <= kappa2 for the stationary kinds)."""
	failures = []
	d, n = 16, 333
	full = E.make_case(layout, d, dt, n, n, True)
	cols = [5, 0, 11]
	il = np.array([0.5, 2.0, 0.25])
	sub = E.sub_columns(full, cols, il)
	rname = "ws" if use_ws else "tile"
	for (name, kind, degree, offset) in VARIANTS[:5]:
		il_k = np.ones(3) if kind == E.LIN else il
		sub_k = E.sub_columns(full, cols, il_k)
		got = run_gram(L, full, kind, degree, use_ws, offset=offset, diag_add=0.04, ldo=n + 3, cols=cols, inv_ls=il_k, d=3)
		if not np.all(got[:, n:] == -7.0):
			failures.append("%s: padding overwritten" % name)
		f = check_values(got[:, :n], sub_k, name + "/cols", kind, degree, offset, use_ws, rname, extra=E.LD(0.04) * np.eye(n, dtype=E.LD))
		if f:
			failures.append(f)
	# combine: K1 = SE on the column subset, then (op) a Matern 5/2 / Matern 3/2 on all columns with the noise on the last item
	k1_true = E.truth_ld(sub, E.SE, 1.1)
	tol1 = E.stationary_bound(sub, E.SE, use_ws, 1.1)
	for op, kind2, kappa2 in ((1, E.M52, 0.9), (2, E.M32, 0.9), (2, E.M12, 0.9)):
		out = torch.full((n, n), -7.0, dtype=TORCH_DT[dt], device="cuda:0")
		run_gram(L, full, E.SE, 0, use_ws, kappa=1.1, out=out, cols=cols, inv_ls=il, d=3)
		got = run_gram(L, full, kind2, 0, use_ws, kappa=kappa2, diag_add=0.04, combine=op, out=out)
		k2_true = E.truth_ld(full, kind2, kappa2)
		tol2 = E.stationary_bound(full, kind2, use_ws, kappa2)
		if op == 1:
			t, tol = k1_true + k2_true, tol1 + tol2 + full.eps * (1.1 + kappa2)
		else:
			t, tol = k1_true * k2_true, tol1 * kappa2 + (1.1 + tol1) * tol2 + full.eps * 1.1 * kappa2
		t = t + E.LD(0.04) * np.eye(n, dtype=E.LD)
		err = float(np.max(np.abs(got.astype(E.LD) - t)))
		print("GRAMEDGE %-6s %s %-18s %-6s d=%-2d same=1  max_abs_err %.3e  bound(max) %.3e  err/bound %.3g" % (
			"se%s%d" % ("+*"[op - 1], kind2), dt, layout, rname, d, err, tol + full.eps, err / (tol + full.eps)))
		if not err <= tol + full.eps:          # (+ eps: the rounding of diag_add onto the diagonal)
			failures.append("combine %d kind %d: %.3e > %.3e" % (op, kind2, err, tol))
	assert not failures, "\n".join(failures)


def run_diag(L, x, dt, kind, degree, inv_ls, kappa, offset, combine=0, out=None, cols=None):
	lib = L.load()
	xd = dev(x, dt)
	ild = dev(inv_ls, dt)
	cd = torch.tensor(list(cols), dtype=torch.int32, device="cuda:0") if cols is not None else None
	if out is None:
		out = torch.full((x.shape[0],), -7.0, dtype=TORCH_DT[dt], device="cuda:0")
	L.check(lib.stpy_gram_diag(abi_kind(kind, degree), L.dtype_code(TORCH_DT[dt]), L.ptr(xd), x.shape[0], x.shape[1], len(inv_ls), L.ptr(cd), L.ptr(ild),
	                           kappa, offset, combine, L.ptr(out), L.stream_ptr()), "gram_diag")
	return out


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("layout", E.LAYOUTS)
def test_gram_diagonal_matches_gram_diag_and_duplicates_give_kappa(L, layout, dt):
	"""a == b: out[i][i] - diag_add equals what stpy_gram_diag returns for the same points, within the bound of the route, with and
	without a workspace; entries of exactly duplicated rows equal kappa within the bound (Matern 1/2: exactly)."""
	failures = []
	n = 384
	for d in E.DIMS:
		case = E.make_case(layout, d, dt, n, n, True)
		dup = [(n // 2 + i, i) for i in range(E.N_DUP)] if layout in ("duplicates", "duplicates_offset") else []
		for (name, kind, degree, offset) in VARIANTS:
			dg = run_diag(L, case.a, dt, kind, degree, case.inv_ls, KAPPA, offset).cpu().numpy().astype(np.float64)
			for use_ws in (False, True):
				got = run_gram(L, case, kind, degree, use_ws, offset=offset, diag_add=0.5)
				tol = tolerance(case, kind, degree, offset, use_ws)
				tol_d = np.diag(tol) if np.ndim(tol) else tol
				with np.errstate(invalid="ignore", over="ignore"):
					ok = np.isfinite(dg) & (np.abs(dg) < float(np.finfo(case.np_dtype).max) / 4)
					diff = np.where(ok, np.abs((np.diag(got) - 0.5) - dg), 0)
					# 0.5 was added in the dtype and is taken off here: one more rounding of the sum
					lim = np.where(ok, np.asarray(tol_d + case.eps * (np.abs(dg) + 0.5), dtype=np.float64), 1)
				worst = float(np.max(diff / lim))
				print("GRAMEDGE %-6s %s %-18s %-6s d=%-2d diag-consistency  max_abs_diff %.3e  err/bound %.3g" % (
					name, dt, layout, "ws" if use_ws else "tile", d, float(diff.max()), worst))
				if worst > 1:
					failures.append("%s d=%d ws=%d: diagonal of stpy_gram and stpy_gram_diag differ by %.3e (%.3g x the bound)" % (name, d, use_ws, float(diff.max()), worst))
				if kind in E.STATIONARY:
					for (i, j) in dup:
						e = abs(got[i, j] - KAPPA)
						if (kind == E.M12 and got[i, j] != np.asarray(KAPPA, dtype=case.np_dtype)) or e > tol:
							failures.append("%s d=%d ws=%d: duplicate rows (%d, %d) give %.17g, kappa is %.17g" % (name, d, use_ws, i, j, got[i, j], KAPPA))
							break
	assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_gram_diag_kinds_cols_mul(L, dt):
	"""stpy_gram_diag for every kind and POLY degree, with `cols`, on cube and offset points, SET then MUL onto the previous result,
	against the diagonal of the truth."""
	failures = []
	m = 77
	for layout in ("cube", "offset"):
		for d, cols in ((3, None), (16, [5, 0, 11, 12])):
			full = E.make_case(layout, d, dt, m, m, True)
			case = full if cols is None else E.sub_columns(full, cols)
			prev_true = np.full(m, 2.0, dtype=E.LD)
			for (name, kind, degree, offset) in VARIANTS:
				t = np.diag(E.truth_ld(case, kind, KAPPA, offset, degree))
				tol = tolerance(case, kind, degree, offset, True)
				tol = np.diag(tol) if np.ndim(tol) else np.full(m, tol, dtype=E.LD)
				with np.errstate(over="ignore", invalid="ignore"):
					ok = np.abs(t) * 2 + tol < E.LD(np.finfo(case.np_dtype).max) / 4
				got = run_diag(L, full.a, dt, kind, degree, case.inv_ls, KAPPA, offset, cols=cols)
				g = got.cpu().numpy().astype(np.float64)
				if np.isnan(g).any() or np.any(np.abs(g.astype(E.LD) - t)[ok] > tol[ok]):
					failures.append("%s %s d=%d SET: %.3e" % (name, layout, d, float(np.max(np.abs(g.astype(E.LD) - t)[ok]))))
				two = torch.full((m,), 2.0, dtype=TORCH_DT[dt], device="cuda:0")
				g2 = run_diag(L, full.a, dt, kind, degree, case.inv_ls, KAPPA, offset, combine=2, out=two, cols=cols).cpu().numpy().astype(np.float64)
				if np.any(np.abs(g2.astype(E.LD) - 2 * t)[ok] > (2 * tol + case.eps * np.abs(2 * t))[ok]):
					failures.append("%s %s d=%d MUL" % (name, layout, d))
				if kind in E.STATIONARY and not np.all(g == np.asarray(KAPPA, dtype=case.np_dtype)):
					failures.append("%s %s d=%d: a stationary diagonal is kappa exactly" % (name, layout, d))
	assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------------------------
def dfactor_slope(kind, r2):
	"""|dF / d(r^2)| per family (see test_lml_weight), in the precision of r2; decreasing in r for all four."""
	r = np.sqrt(r2)
	if kind == E.SE:
		return np.exp(-r2 / 2) / 2
	if kind == E.M12:
		return (1 + r) * np.exp(-r) / (2 * r * r2)
	if kind == E.M32:
		s3 = np.sqrt(r2.dtype.type(3))
		return 3 * s3 * np.exp(-s3 * r) / (2 * r)
	s5 = np.sqrt(r2.dtype.type(5))
	return np.exp(-s5 * r) * 25 / 6


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("layout", ["cube", "offset", "duplicates", "duplicates_offset"])
def test_lml_weight(L, layout, dt):
	"""stpy_lml_weight directly: H = (w Kinv - alpha alpha^T) o kappa F with a random symmetric Kinv and a random alpha, given
	separately and in place (Kinv == NULL), for SE and Matern 1/2, 3/2, 5/2.

	F and |dF/d(r^2)| per family, t = sqrt(3) r resp. sqrt(5) r:
	  SE          F = exp(-r^2/2)           |dF/dr^2| = exp(-r^2/2) / 2             <= 1/2
	  Matern 5/2  F = 5/3 (1 + t) exp(-t)   |dF/dr^2| = 25/6 exp(-t)                <= 25/6
	  Matern 3/2  F = 3 exp(-t)             |dF/dr^2| = 3 sqrt(3) exp(-t) / (2 r)   unbounded at r = 0
	  Matern 1/2  F = exp(-r) / r           |dF/dr^2| = (1 + r) exp(-r) / (2 r^3)   unbounded at r = 0
	So Matern 3/2 and 1/2 have no finite constant: where the norm expansion cannot resolve r (r^2 within a few delta of zero, delta =
	4 (d + 3) eps D^2 the r^2 term of the Gram bound) nothing can be asked of F itself.  All four slopes decrease in r, so off that
	neighbourhood (r^2 >= 32 delta, where the computed r^2 is at least half the true one) the mean-value bound with the slope taken at
	r^2 / 2 holds entry by entry:
	    |H_ij - H_true,ij| <= kappa (|G_ij| (slope(r_ij^2 / 2) delta + 8 eps max(F_ij, 1)) + 3 eps (|w Kinv_ij| + |alpha_i alpha_j|) F_ij)
	(G = w Kinv - alpha alpha^T; the last term is its own rounding).  For SE and Matern 5/2 that is at most the Gram bound with c_kind
	replaced by 1/2 resp. 25/6, times max |G|.
	What the gradient consumes is sum_ij H_ij u_ijm^2 per coordinate m, and |dF/dr^2| u^2 <= |dF/dr^2| r^2 is bounded for Matern 3/2
	and grows only like 1 / (2 r) for Matern 1/2, so the contracted sums are held to the sum of the entry bounds times u_ijm^2 over ALL
	pairs: inside the neighbourhood a pair may contribute up to |G_ij| kappa u^2 (2 F_true + 1 / sqrt(eps D^2)) -- F no larger than what
	the rounding noise of r^2 itself allows -- and F_true u^2 is 0 on coincident pairs, where H only has to be finite."""
	lib = L.load()
	failures = []
	tdt = TORCH_DT[dt]
	for d, n in ((3, 256), (16, 257)):
		case = E.make_case(layout, d, dt, n, n, True)
		rng = np.random.RandomState(17 * d + n)
		Kinv = rng.normal(size=(n, n)); Kinv = (Kinv + Kinv.T).astype(case.np_dtype).astype(np.float64)
		alpha = rng.normal(size=n).astype(case.np_dtype).astype(np.float64)
		w = 0.75
		G = (E.LD(w) * Kinv.astype(E.LD) - np.outer(alpha, alpha).astype(E.LD))
		Gabs = np.abs(E.LD(w) * Kinv.astype(E.LD)) + np.abs(np.outer(alpha, alpha).astype(E.LD))
		r2, _, _ = E.sq_dist_and_dot(case)
		D2 = E.diameter_sq(case)
		delta = E.LD(4.0 * (d + 3) * case.eps * D2)
		coincident = r2 == 0
		near = (~coincident) & (r2 < 32 * delta)
		far = ~(coincident | near)
		a_ld, il_ld = case.a.astype(E.LD), case.inv_ls.astype(E.LD)
		xd, ild, ald = dev(case.a, dt), dev(case.inv_ls, dt), dev(alpha, dt)
		ws = workspace(L, n, n, d, dt)
		for (name, kind, _, _) in VARIANTS[:4]:
			with np.errstate(divide="ignore", invalid="ignore"):
				F = np.where(coincident, 0, E.dfactor_of_r2(kind, np.where(coincident, 1, r2)))
				slope = dfactor_slope(kind, np.where(coincident, 1, r2) / 2)
			entry_tol = E.LD(KAPPA) * (np.abs(G) * (slope * delta + 8 * case.eps * np.maximum(F, 1)) + 3 * case.eps * Gabs * F)
			entry_tol = np.where(near, E.LD(KAPPA) * np.abs(G) * (2 * F + 1 / np.sqrt(E.LD(case.eps * D2))), entry_tol)
			H_true = E.LD(KAPPA) * G * F
			for in_place in (False, True):
				Kd = dev(Kinv, dt)
				Hd = Kd if in_place else torch.full((n, n), -7.0, dtype=tdt, device="cuda:0")
				L.check(lib.stpy_lml_weight(kind, L.dtype_code(tdt), L.ptr(xd), n, d, d, None, L.ptr(ild), KAPPA, w, L.ptr(ald),
				                            None if in_place else L.ptr(Kd), n, L.ptr(Hd), n, L.ptr(ws), ws.numel(), L.stream_ptr()), "lml_weight")
				H = Hd.cpu().numpy().astype(np.float64)
				tag = "%s %s d=%d %s" % (name, layout, d, "in place" if in_place else "Kinv given")
				if not np.all(np.isfinite(H)):
					failures.append(tag + ": non-finite H")
					continue
				err = np.abs(H.astype(E.LD) - H_true)
				ratio = float(np.max(np.where(far, err / entry_tol, 0)))
				worst_c = 0.0
				for m in range(d):
					u = (a_ld[:, m, None] - a_ld[None, :, m]) * il_ld[m]
					u2 = u * u
					got_m = np.sum(H.astype(E.LD) * u2)
					true_m = np.sum(H_true * u2)
					tol_m = np.sum(entry_tol * u2)
					worst_c = max(worst_c, float(abs(got_m - true_m) / tol_m))
				print("GRAMEDGE %-6s %s %-18s lml_weight d=%-2d %-10s  H err/bound %.3g (max_abs_err %.3e)  contracted err/bound %.3g" % (
					name, dt, layout, d, "in-place" if in_place else "Kinv", ratio, float(np.max(np.where(far, err, 0))), worst_c))
				if ratio > 1:
					failures.append(tag + ": H is %.3g x the entry bound off the coincident pairs" % ratio)
				if worst_c > 1:
					failures.append(tag + ": sum_ij H_ij u_ijm^2 is %.3g x its bound" % worst_c)
	assert not failures, "\n".join(failures)


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("dt,tol", [("f64", 1e-12), ("f32", 2e-4)])
def test_scaled_points_gemm_and_lml_grad_reduce_off_centre(L, dt, tol, centred):
	"""The chain the evidence gradient runs -- stpy_scaled_points_t, P = H [Xs | 1] (stpy_gemm_nt), stpy_lml_grad_reduce -- on the
	`offset` layout: the per-coordinate sums against inv_ls_k / 2 sum_ij H_ij (u_ik - u_jk)^2 in longdouble, relative to sum |H|, at the
	tolerance of test_gpu_kernels.py::test_scaled_points_and_lml_grad_reduce.  centred: the form GaussianProcess uses, the operand
	relative to the first point (ones_row = 3, exact on these inputs) into stpy_lml_grad_reduce_centred."""
	lib = L.load()
	tdt = TORCH_DT[dt]
	code = L.dtype_code(tdt)
	reduce = lib.stpy_lml_grad_reduce_centred if centred else lib.stpy_lml_grad_reduce
	failures = []
	for d in (3, 16):
		n = 700
		case = E.make_case("offset", d, dt, n, n, True)
		rng = np.random.RandomState(5 + d)
		H = rng.normal(size=(n, n)); H = (H + H.T).astype(case.np_dtype).astype(np.float64)
		xd, ild, Hd = dev(case.a, dt), dev(case.inv_ls, dt), dev(H, dt)
		XT = torch.empty((d + 1, n), dtype=tdt, device="cuda:0")
		L.check(lib.stpy_scaled_points_t(code, L.ptr(xd), n, d, d, None, L.ptr(ild), L.ptr(XT), n, 3 if centred else 1, L.stream_ptr()), "scaled_points_t")
		want = ((case.a - case.a[0]) if centred else case.a) * case.inv_ls          # powers of two, integer offsets: exact in the dtype
		got_xt = XT.cpu().numpy().astype(np.float64)
		if not (np.array_equal(got_xt[:d], want.T) and np.all(got_xt[d] == 1.0)):
			failures.append("d=%d: stpy_scaled_points_t(ones_row=%d) is not the %sscaled points" % (d, 3 if centred else 1, "centred " if centred else ""))
		P = torch.empty((n, d + 1), dtype=tdt, device="cuda:0")
		L.check(lib.stpy_gemm_nt(code, n, d + 1, n, L.ptr(Hd), n, L.ptr(XT), n, L.ptr(P), d + 1, 0, 0, L.stream_ptr()), "gemm_nt")
		acc = torch.zeros((d,), dtype=tdt, device="cuda:0")
		L.check(reduce(code, L.ptr(xd), n, d, d, None, L.ptr(ild), L.ptr(P), d + 1, None, L.ptr(acc), L.stream_ptr()), "lml_grad_reduce")
		got = acc.cpu().numpy().astype(np.float64)
		a_ld, il_ld, H_ld = case.a.astype(E.LD), case.inv_ls.astype(E.LD), H.astype(E.LD)
		scale = float(np.abs(H).sum())
		for k in range(d):
			u = (a_ld[:, k, None] - a_ld[None, :, k]) * il_ld[k]
			ref = float(il_ld[k] * np.sum(H_ld * u * u) / 2)
			rel = abs(got[k] - ref) / scale
			print("GRAMEDGE lml_grad_reduce %s %s offset d=%-2d k=%-2d rel_err %.3e (tolerance %.1e)" % ("centred" if centred else "plain", dt, d, k, rel, tol))
			if not rel < tol:
				failures.append("d=%d coordinate %d: %.3e" % (d, k, rel))
	assert not failures, "\n".join(failures)
