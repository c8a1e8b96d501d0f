"""
CPU self-check of tests/gram_edge_cases.py: keeps the GPU edge tests honest (a correct evaluation fits the derived bounds with room)
and makes sure they have teeth (the uncentred norm expansion does not fit them once the data leaves the origin).  No GPU.
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import gram_edge_cases as E

N, Q = 256, 384
EXPANSION_KINDS = (E.SE, E.M32, E.M52)


def test_inputs_are_exact_and_translations_keep_the_differences():
	for dt in E.DTYPES:
		for d in E.DIMS:
			base = E.make_case("cube", d, dt, 64, 48)
			for layout in E.LAYOUTS:
				c = E.make_case(layout, d, dt, 64, 48)
				assert np.array_equal(c.a.astype(c.np_dtype).astype(np.float64), c.a) and np.array_equal(c.b.astype(c.np_dtype).astype(np.float64), c.b)
			# an offset layout is the pow-2-lengthscale cube moved by integers: same generator stream, so same grid points
			off = E.make_case("offset", d, dt, 64, 48)
			assert np.all(np.abs(off.a - E.OFFSET[dt]) <= 1.0) and np.all((off.a * E.GRID[dt]) % 1 == 0)
			assert base.a.shape == off.a.shape


@pytest.mark.parametrize("dt", sorted(E.DTYPES))
@pytest.mark.parametrize("layout", E.LAYOUTS)
def test_shifted_and_direct_fit_the_bound_and_raw_does_not(layout, dt):
	"""Per layout and dtype, for every d: the shifted norm expansion (a[0] subtracted first) stays within the expansion bound and direct
	differences within the direct bound, both with 4x headroom; the raw expansion exceeds the bound 10x on the offset layouts."""
	for d in E.DIMS:
		for same in (False, True):
			c = E.make_case(layout, d, dt, N, N if same else Q, same)
			for kind in EXPANSION_KINDS:
				bound = E.expansion_bound(c, kind)
				e_shift = E.emulated_error(c, kind, "shifted")
				assert e_shift * 4 <= bound, (d, same, kind, e_shift, bound)
				if layout in E.OFFSET_LAYOUTS:
					e_raw = E.emulated_error(c, kind, "raw")
					assert e_raw >= 10 * bound, (d, same, kind, e_raw, bound)
			for kind in (E.M12, E.M32, E.M52):
				e_dir = E.emulated_error(c, kind, "direct")
				assert e_dir * 4 <= E.direct_bound(c), (d, same, kind, e_dir, E.direct_bound(c))
				assert e_dir * 4 <= E.expansion_bound(c, E.SE), (d, same, kind)


@pytest.mark.parametrize("dt", sorted(E.DTYPES))
def test_tiny_lengthscale_reaches_the_denormal_and_the_flushed_band(dt):
	"""Every family has entries whose truth is a denormal of the dtype and entries below its smallest denormal; and entries of order one."""
	fi = np.finfo(E.DTYPES[dt])
	tiny, sub = E.LD(fi.tiny), E.LD(fi.tiny) * E.LD(fi.eps)
	for d in E.DIMS:
		for same in (False, True):
			c = E.make_case("tiny_lengthscale", d, dt, N, N if same else Q, same)
			for kind in E.STATIONARY:
				t = E.truth_ld(c, kind)
				assert np.any((t < tiny) & (t >= sub)), (d, same, kind)
				assert np.any(t < sub), (d, same, kind)
				assert np.any(t > 0.5), (d, same, kind)


def test_huge_lengthscale_is_kappa_to_a_few_digits():
	"""inv_ls = 2^-20: r <= 2 sqrt(d) 2^-20, so the smooth families sit within r^2 ~ 1e-10 of kappa and Matern 1/2 within r ~ 1e-5; the GPU
	test holds the kernels to the truth at the bound and to kappa at the bound plus this distance."""
	for dt in E.DTYPES:
		for d in E.DIMS:
			c = E.make_case("huge_lengthscale", d, dt, N, Q)
			for kind in E.STATIONARY:
				dev = np.max(np.abs(E.truth(c, kind, 1.3) - 1.3))
				assert dev <= 1.3 * (2e-5 if kind == E.M12 else 1e-9), (dt, d, kind, dev)


@pytest.mark.parametrize("d", E.DIMS)
def test_truth_matches_the_pinned_oracle_on_cube(d):
	c = E.make_case("cube", d, "f64", 257, 513)
	ls = 1.0 / c.inv_ls
	assert np.max(np.abs(E.truth(c, E.SE, 1.3) - O.ard(c.a, c.b, ls, 1.3))) < 1e-13
	for kind, nu in ((E.M12, 0.5), (E.M32, 1.5), (E.M52, 2.5)):
		assert np.max(np.abs(E.truth(c, kind, 1.3) - O.ard_matern(c.a, c.b, ls, nu, 1.3))) < 1e-13
	one = E.sub_columns(c, range(d), np.ones(d))
	assert np.max(np.abs(E.truth(one, E.LIN, 1.3, 0.25) - O.linear(c.a, c.b, 1.3, 0.25))) < 1e-13
	for p in E.POLY_DEGREES:
		ref = O.polynomial(c.a, c.b, p, 1.3)
		assert np.max(np.abs(E.truth(one, E.POLY, 1.3, 1.0, p) - ref)) < 1e-13 * np.max(np.abs(ref))


def test_dot_kind_bound_holds_for_a_dtype_evaluation():
	"""LINEAR / POLY evaluated in the dtype with sequential sums stay inside their bound on cube and offset."""
	for dt in E.DTYPES:
		T = E.DTYPES[dt]
		for layout in ("cube", "offset"):
			for d in E.DIMS:
				c = E.make_case(layout, d, dt, 96, 80)
				xa, xb = (c.a.astype(T) * c.inv_ls.astype(T)), (c.b.astype(T) * c.inv_ls.astype(T))
				dot = np.zeros((c.q, c.n), dtype=T)
				for k in range(d):
					dot += xb[:, k, None] * xa[None, :, k]
				for p in E.POLY_DEGREES:
					with np.errstate(over="ignore"):
						s = dot + T(1.0)
						v = np.ones_like(s)
						for _ in range(p):
							v = v * s
						v = T(1.3) * v
					t = E.truth_ld(c, E.POLY, 1.3, 1.0, p)
					ok = np.abs(t) < E.LD(np.finfo(T).max) / 4
					err = np.abs(v.astype(E.LD) - t)[ok]
					assert np.all(err <= E.dot_kind_bound(c, E.POLY, 1.3, 1.0, p)[ok]), (dt, layout, d, p)
				lin = T(1.3) * dot + T(0.25)
				assert np.all(np.abs(lin.astype(E.LD) - E.truth_ld(c, E.LIN, 1.3, 0.25)) <= E.dot_kind_bound(c, E.LIN, 1.3, 0.25))
