"""
CPU self-check of tests/gram_grad_cases.py: the cases of tests/test_gpu_gram_grad_edges.py tell a right evaluation of stpy_gram_grad from a
wrong one before any GPU time is spent.  The oracle agrees with central differences of the longdouble kernel truth of
tests/gram_edge_cases.py; a numpy evaluator in the dtype that subtracts the coordinates before it scales them stays inside the bound on
every case and gives the same bits on every twin; each planted error (gram_grad_cases.PLANTS) exceeds the bound, breaks the twin identity
or leaves a NaN on the cases that gram_grad_cases.DEFEATS names.  `-s` prints, case by case, which planted evaluators it defeats.  No GPU.
"""
import numpy as np
import pytest

from tests import gram_edge_cases as E
from tests import gram_grad_cases as C

DTS = sorted(E.DTYPES)
LD = E.LD
WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def test_plan_mirrors_the_kernel():
	"""grad_plan of csrc/grad.hip at the shapes the cases cut it at: (Q, output blocks, chunk, chunks, tiles of test rows)."""
	assert C.plan(5, 1, 3, 1) == (3, 1, 256, 1, 2)
	assert C.plan(5, 256, 3, 1) == (3, 1, 256, 1, 2)
	assert C.plan(5, 257, 3, 1) == (3, 1, 256, 2, 2)
	assert C.plan(5, 513, 3, 1) == (3, 1, 256, 3, 2)
	assert C.plan(37, 1000, 33, 1) == (33, 3, 256, 4, 10)
	assert C.plan(5, 257, 4, 2) == (20, 2, 256, 2, 2)
	assert C.plan(4096, 65536, 16, 1) == (16, 1, 32768, 2, 1024)


def _value(gc, xt):
	"""sum_i c_ti k(xt_t, x_i) from the kernel truth of gram_edge_cases, (m,) longdouble."""
	case = E.Case("fd", gc.d, gc.dt, np.ascontiguousarray(gc.x[:, gc.sel]), np.ascontiguousarray(xt[:, gc.sel]), gc.inv_ls, False)
	return np.sum(gc.coef_ld() * E.truth_ld(case, gc.kind, gc.kappa, gc.offset, gc.degree), axis=1)


@pytest.mark.skipif(not WIDER, reason="numpy.longdouble is no wider than float64 here")
@pytest.mark.parametrize("family", sorted(C.FAMILIES))
def test_oracle_against_central_differences(family):
	"""G against (f(xt + h e_k) - f(xt - h e_k)) / 2 h of the kernel truth, H against the same difference of the oracle's own G, h = 2^-20,
	relative 1e-9 of the sum of absolute values of the terms (truncation h^2 f''' / 6 and round-off eps / h are both near 1e-13 in 80-bit
	arithmetic).  Random cube points: no pair is near r = 0, where Matern 1/2 and 3/2 have no third derivative.  Once plain, once through a
	column subset of a wider x."""
	h = 2.0 ** -20
	order = 2 if family in C.HESSIAN_FAMILIES else 1
	plain = C.GradCase("fd", family, "f64", *C._cube(3, "f64", 11, 3), order=order)
	w, cols, g = C.D.wide_case("cube", 5, "f64", 9, 3)
	wide = C.GradCase("fd-cols", family, "f64", w.a, w.b, g.inv_ls, cols=cols, order=order)
	for gc in (plain, wide):
		o = C.oracle(gc)
		r2 = E.sq_dist_and_dot(E.Case("r", gc.d, "f64", gc.x[:, gc.sel], gc.xt[:, gc.sel], gc.inv_ls, False))[0]
		assert float(np.min(r2)) > 1e-3
		for k, ck in enumerate(gc.sel):
			up, dn = gc.xt.copy(), gc.xt.copy()
			up[:, ck] += h
			dn[:, ck] -= h
			fd = (_value(gc, up) - _value(gc, dn)) / (2 * LD(h))
			assert np.all(np.abs(fd - o["G"][:, k]) <= 1e-9 * o["S_G"][:, k]), (family, gc.name, k)
			if order == 2:
				gu = C.oracle(C.GradCase("u", family, "f64", gc.x, up, gc.inv_ls, cols=gc.cols, coef_key=gc.name))["G"]
				gd = C.oracle(C.GradCase("d", family, "f64", gc.x, dn, gc.inv_ls, cols=gc.cols, coef_key=gc.name))["G"]
				fdh = (gu - gd) / (2 * LD(h))
				assert np.all(np.abs(fdh - o["H"][:, k, :]) <= 1e-9 * np.maximum(o["S_H"][:, k, :], o["S_G"])), (family, gc.name, k)
				assert np.array_equal(o["H"], np.transpose(o["H"], (0, 2, 1)))


def _defeat(gc, base, plant):
	"""How the planted evaluator fails on the case: "nan", "bound", "twin" (several, joined by +), or "" if it passes."""
	Gb, Hb = C.evaluate(gc, plant)
	r = C.check(gc, Gb, Hb)
	how = []
	if not np.isfinite(r["ratio"]):
		how.append("nan")
	elif r["ratio"] > 1.0:
		how.append("bound")
	if base is not None:
		G0, H0 = C.evaluate(base, plant)
		if not (np.array_equal(Gb, G0) and (Hb is None or np.array_equal(Hb, H0))):
			how.append("twin")
	return "+".join(how)


def _applies(plant, gc):
	"""The cases on which a plant changes the arithmetic at all."""
	if plant in ("scale_first", "norm_expansion"):
		return not gc.dot and (gc.twin_of is not None or gc.name.startswith(("cube", "duplicates")))
	if plant == "m12_unguarded":
		return gc.family == "m12"
	if plant == "inv_ls_by_col":
		return gc.cols is not None
	if plant == "no_w1_diag":
		return gc.order == 2 and not gc.dot
	if plant == "swap_uv":
		return gc.u is not None or gc.v is not None
	if plant == "drop_last_tile":
		return gc.m % C.GG_TM != 0
	return gc.name.startswith(("plan", "cube"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", sorted(C.FAMILIES))
def test_cases_tell_right_from_wrong(family, dt):
	cs = C.cases(dt, family)
	by_name = {gc.name: gc for gc in cs}
	worst, c_eff, defeated = 0.0, 0.0, set()
	for gc in cs:
		base = by_name[gc.twin_of] if gc.twin_of else None
		Gb, Hb = C.evaluate(gc)
		r = C.check(gc, Gb, Hb)
		worst, c_eff = max(worst, r["ratio"]), max(c_eff, C.c_effective(gc))
		assert r["ratio"] <= 1.0, (gc.name, r)
		assert r["untouched"], gc.name
		if base is not None:
			G0, H0 = C.evaluate(base)
			assert np.array_equal(Gb, G0) and (Hb is None or np.array_equal(Hb, H0)), "%s: subtract-first is not bit-equal on the twin" % gc.name
			assert np.array_equal(C.oracle(gc)["G"], C.oracle(base)["G"]), "%s: the twin has another truth" % gc.name
		if gc.name.startswith("exact"):
			assert r["exact_zero_G"] and r.get("exact_zero_offdiag_H", True), gc.name
		line = []
		for plant in C.PLANTS:
			if _applies(plant, gc):
				how = _defeat(gc, base, plant)
				if how:
					line.append("%s (%s)" % (plant, how))
					defeated.update((plant, gc.name, h) for h in how.split("+"))
		print("GRADCASES %-44s defeats: %s" % (gc.name, ", ".join(line) if line else "-"))
	print("GRADCASES %s %s: %d cases, subtract-first largest error / bound %.3g, largest c %.1f" % (family, dt, len(cs), worst, c_eff))
	for plant in C.PLANTS:
		for (name, how) in C.DEFEATS[plant]:
			if name in by_name:
				assert (plant, name, how) in defeated, "%s should defeat %s by %s" % (name, plant, how)
	E.make_case.cache_clear()


def test_every_plant_is_named_in_both_dtypes_and_every_name_exists():
	names = {gc.name for dt in DTS for family in C.FAMILIES for gc in C.cases(dt, family)}
	for plant in C.PLANTS:
		assert C.DEFEATS[plant], plant
		for dt in DTS:
			assert any("-%s" % dt in name for name, _ in C.DEFEATS[plant]), (plant, dt)
		for name, how in C.DEFEATS[plant]:
			assert name in names, name
			assert how in ("bound", "twin", "nan")
	assert all(how == "twin" or name.split("-")[0].count("+") for name, how in C.DEFEATS["scale_first"]), "scale-first is judged on the twins"
	E.make_case.cache_clear()


@pytest.mark.parametrize("dt", DTS)
def test_exact_cases_have_the_closed_form(dt):
	"""n = m = 1, xt == x: the oracle's G is 0 and its H is c psi(0) inv_ls_k^2 on the diagonal (psi(0) = -kappa for SE, -(5 / 3) kappa for
	Matern 5/2), 0 off it."""
	for family, psi0 in (("se", LD(-1)), ("m52", LD(-5) / 3)):
		gc, = C.exact_cases(dt, family)
		o = C.oracle(gc)
		c = LD(gc.u[0]) * LD(gc.alpha[0])
		assert np.all(o["G"] == 0) and np.all(o["S_G"] == 0)
		want = np.diag(c * psi0 * LD(gc.kappa) * gc.inv_ls.astype(LD) ** 2)
		assert np.all(np.abs(o["H"][0] - want) <= 4 * np.finfo(np.longdouble).eps * np.abs(want))
		assert np.all(o["H"][0][~np.eye(3, dtype=bool)] == 0)
	for family in ("m12", "m32"):
		gc, = C.exact_cases(dt, family)
		assert np.all(C.oracle(gc)["G"] == 0)


def test_duplicates_layout_has_coincident_and_one_step_pairs():
	"""Test rows 3 .. 14 copy training rows 0 .. 11; rows 15 .. 20 sit one grid step from training rows 12 .. 17."""
	for dt in DTS:
		gc = {c.name: c for c in C.layout_cases(dt, "m12")}["duplicates-m12-%s-d3-o1" % dt]
		assert np.array_equal(gc.xt[3:3 + E.N_DUP], gc.x[:E.N_DUP])
		diff = gc.xt[3 + E.N_DUP:3 + E.N_DUP + E.N_NEAR] - gc.x[E.N_DUP:E.N_DUP + E.N_NEAR]
		assert np.all(np.sum(diff != 0, axis=1) == 1) and np.all(np.abs(diff).sum(axis=1) == 1.0 / E.GRID[dt])
	E.make_case.cache_clear()
