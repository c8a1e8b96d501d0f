"""
CPU self-check of tests/direct_eval_cases.py: the cases of tests/test_gpu_direct_eval_edges.py tell a right direct-difference evaluator from
a wrong one before any GPU time is spent.  A subtract-first evaluation in the dtype fits kappa (d + 8) eps on every layout and gives the same
bits on a layout and its off-centre twin; a scale-first one misses the bound by at least a factor 2 on the twins named by
``direct_eval_cases.discriminates``; the two oracles (longdouble truth, nystrom_oracle.kernel with a lengthscale vector) agree; the lattice
and the nearly-flat case behave on the oracle's pivoted Cholesky as the GPU tests expect of the device.  No GPU.
"""
import numpy as np
import pytest

from tests import direct_eval_cases as D
from tests import gram_edge_cases as E
from tests import nystrom_oracle as NO

DTS = sorted(E.DTYPES)


def test_ard_vectors_are_distinct_spread_and_round_trip():
	for dt in DTS:
		for d in D.DIMS + (2,):
			v = D.ard_inv_ls(d, dt)
			assert v.shape == (d,) and len(set(v.tolist())) == d
			assert np.all(v * np.sqrt(d) >= 0.3) and np.all(v * np.sqrt(d) <= 1.5)
			if d > 1:
				assert v.max() >= 4 * v.min()
			if d > 2:
				assert np.any(np.diff(v) > 0) and np.any(np.diff(v) < 0)
			assert np.array_equal((1.0 / (1.0 / v)).astype(E.DTYPES[dt]).astype(np.float64), v)
	for d in (12, 20, 33):
		w, cols, g = D.wide_case("cube", d, "f64", 16, 16, True)
		assert len(set(cols)) == d and max(cols) < 40 and np.any(np.diff(cols) > 0) and np.any(np.diff(cols) < 0)
		assert np.array_equal(g.a, w.a[:, cols]) and np.array_equal(g.inv_ls, D.ard_inv_ls(d, "f64"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", D.DIMS)
def test_the_two_oracles_agree_and_the_orders_separate(d, dt):
	"""Per d and dtype, on both shapes and every layout of the entry tests: nystrom_oracle.kernel (float64, per-coordinate lengthscales) is
	within direct_bound of the longdouble truth; subtract-first stays within the bound, with 4x headroom, and is bit-equal to its
	value on the centred layout; scale-first exceeds the bound at least twice on the discriminating twins."""
	for (n, q, same) in D.SHAPES:
		r2_of = {}
		for name, case, base in D.entry_cases(d, dt, n, q, same):
			bound = E.direct_bound(case)
			r2 = D.emulate_r2(case, "subtract_first")
			r2_of[name] = (r2, E.sq_dist_and_dot(case)[0])
			if base is not None:
				assert np.array_equal(r2, r2_of[base][0]), (name, "subtract-first is not bit-equal on the twin")
				assert np.array_equal(r2_of[name][1], r2_of[base][1]), (name, "the twin has another truth")
			for kind in D.KINDS:
				t = E.truth(case, kind, 1.0)
				assert np.max(np.abs(D.oracle_kernel(case, kind) - t)) <= bound, (name, kind)
				e_sub = D.order_error(case, kind, "subtract_first")
				assert e_sub * 4 <= bound, (name, kind, e_sub, bound)
				if D.discriminates(name, d, dt):
					e_scale = D.order_error(case, kind, "scale_first")
					assert e_scale >= 2 * bound, (name, kind, same, e_scale / bound)
	E.make_case.cache_clear()


def test_every_dimension_has_a_discriminating_twin_in_both_dtypes():
	for dt in DTS:
		for d in D.DIMS:
			names = [name for name, _, _ in D.entry_cases(d, dt, *D.SHAPES[0])]
			assert any(D.discriminates(name, d, dt) for name in names), (dt, d)
	E.make_case.cache_clear()


def test_coincident_and_one_step_pairs_of_the_duplicates_layout():
	"""12 exact copies (truth exactly kappa) and 6 pairs one grid step apart.  In float64 a step of 2^-30 gives r of about 5e-10: Matern 1/2
	is 1 - r, well below 1; Matern 3/2 and 5/2 are 1 - O(r^2) = 1 - 4e-19, which ROUNDS to 1 in float64, so only `<= kappa` can be asked
	of them there (the GPU test asks `< kappa` wherever the rounded truth is below kappa)."""
	for d in D.DIMS:
		c = D.ard_case("duplicates", d, "f64", 129, 129, True)
		h = c.n // 2
		dup = (np.arange(h, h + E.N_DUP), np.arange(E.N_DUP))
		near = (np.arange(h + E.N_DUP, h + E.N_DUP + E.N_NEAR), np.arange(E.N_DUP, E.N_DUP + E.N_NEAR))
		r2, _, _ = E.sq_dist_and_dot(c)
		assert np.all(r2[dup] == 0) and np.all(r2[near] > 0)
		for kind in D.KINDS:
			t = E.truth(c, kind, 1.0)
			assert np.all(t[dup] == 1.0)
			assert np.all(t[near] < 1.0) if kind == E.M12 else np.all(t[near] == 1.0)


def test_ard_kernel_objects_pair_lengthscales_with_the_group_columns():
	"""What the two matrix-free classes hand to the device for an `ard` / `ard_matern` kernel object that reads a shuffled `group` of a
	40-wide x: column group[k] with 1 / ard_gamma[group[k]], in the order of the group -- the very inv_ls of the case (host only)."""
	import torch
	from stpy_amd import KernelFunction
	from stpy_amd.continuous_processes.nystrom_fea import _stationary_term
	_, cols, g = D.wide_case("cube", 20, "f64", 16, 16, True)
	wide_gamma = np.ones(40)
	wide_gamma[cols] = D.gamma_of(g)
	for name, kind in (("ard", E.SE), ("ard_matern", E.M32)):
		t = _stationary_term(KernelFunction(kernel_name=name, ard_gamma=torch.from_numpy(wide_gamma), nu=1.5, kappa=1.3, d=40, group=list(cols)))
		assert t['kind'] == kind and t['kappa'] == 1.3 and list(t['group']) == cols
		assert np.array_equal(np.array(t['inv_ls']), g.inv_ls)
	t = _stationary_term(KernelFunction(kernel_name="ard", ard_gamma=torch.from_numpy(D.gamma_of(D.ard_case("cube", 3, "f64", 16, 16))), d=3))
	assert list(t['group']) == [0, 1, 2] and np.array_equal(np.array(t['inv_ls']), D.ard_inv_ls(3, "f64"))


@pytest.mark.parametrize("dt", DTS)
def test_lattice_on_the_oracle(dt):
	"""K = kappa I exactly: the oracle's pivoted Cholesky at kappa = 4 takes the pivots 0 .. 299 in order, Ft[j] = 2 e_j, dres = 0 on the
	pivots and 4 elsewhere, in both dtypes and all four kinds."""
	c = D.lattice_case(dt)
	T = c.np_dtype
	for kind in D.KINDS:
		K = E.truth(c, kind, D.LATTICE_KAPPA)
		assert np.array_equal(K, D.LATTICE_KAPPA * np.eye(c.n))
		assert np.array_equal(D.oracle_kernel(c, kind, D.LATTICE_KAPPA, T), K.astype(T))
		piv, Ft, dres, rank = NO.pivoted_cholesky(D.KIND_NAME[kind], c.a.astype(T), D.gamma_of(c), D.LATTICE_M, kappa=D.LATTICE_KAPPA, dtype=T)
		assert rank == D.LATTICE_M and np.array_equal(piv, np.arange(D.LATTICE_M))
		want = np.zeros((D.LATTICE_M, c.n), dtype=T)
		want[np.arange(D.LATTICE_M), np.arange(D.LATTICE_M)] = 2
		assert Ft.dtype == T and np.array_equal(Ft, want)
		assert np.all(dres[:D.LATTICE_M] == 0) and np.all(dres[D.LATTICE_M:] == 4)


@pytest.mark.parametrize("dt", DTS)
def test_nearly_flat_on_the_oracle(dt):
	"""inv_ls = 2^-20: the oracle stops at rank 1 for SE, Matern 3/2 and 5/2, the first pivot (kappa = 1) and the second residual two orders
	of magnitude on either side of the tolerance."""
	c = D.flat_case(dt)
	T = c.np_dtype
	tol = D.FLAT_TOL[dt]
	assert c.n == D.FLAT_N and c.d == D.FLAT_D and np.all(c.inv_ls == 2.0 ** -20)
	for kind in D.FLAT_KINDS:
		tr = []
		piv, Ft, dres, rank = NO.pivoted_cholesky(D.KIND_NAME[kind], c.a.astype(T), D.gamma_of(c), 8, tol=tol, dtype=T, trace=tr)
		print("nearly flat %s %s: second residual %.3e, tolerance %.1e" % (dt, D.KIND_NAME[kind], tr[1][1], tol))
		assert rank == 1 and piv[0] == 0 and np.all(piv[1:] == -1) and np.all(Ft[1:] == 0)
		assert tr[0][0] >= 100 * tol and 0 <= tr[1][1] <= tol / 100
		assert np.abs(dres).max() <= tol and dres[0] == 0
