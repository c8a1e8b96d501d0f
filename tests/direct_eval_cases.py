"""
Inputs for the edge tests of the direct-difference kernel evaluator (pc_phi and the distance loops of csrc/pchol.hip and csrc/kmv.hip: stpy_pchol,
stpy_kmv, stpy_pcg and the two matrix-free classes).  Built on tests/gram_edge_cases.py (grids, offsets, longdouble truth, direct_bound) and
tests/nystrom_oracle.py; plain numpy, no GPU code, no library.  tests/test_direct_eval_cases_cpu.py checks on the CPU that these cases can
tell a right evaluator from a wrong one; tests/test_gpu_direct_eval_edges.py runs them on the device.

The contract under test: a value is within kappa (d + 8) eps of the truth WHEREVER the data lies, exactly kappa on coincident points, bitwise
symmetric, and the coordinates are subtracted before they are scaled by the inverse lengthscale.

ARD inverse lengthscales.  A shuffled geometric ladder from 0.31 / sqrt(d) to 1.45 / sqrt(d) (a spread of 4.7; the interior rungs jittered by
a fraction of a rung), rounded to the dtype: in the range uniform(0.3, 1.5) / sqrt(d) of the Gram suite, never a power of two (scaling rounds),
distinct with neighbouring values at least 1% apart and not monotone in the coordinate index, so any permutation, repeat or shift of the
vector moves kernel values by far more than the bound.  In float64 the vector is chosen so that 1 / (1 / inv_ls) == inv_ls: the oracle, which
takes lengthscales, then computes with the very numbers the device gets.

Twins.  A centred layout of gram_edge_cases (cube, duplicates: dyadic grid points in [-1, 1]) and its translate by integers: "offset" (E.OFFSET
in every column), "offset_per_column" (round(E.OFFSET (k + 1) / d) in column k) and "offset_far" (1000 in every column; float32 only, where
E.OFFSET is 100: 1000 + k / 1024 needs 21 of 24 bits).  Both members are exact in the dtype and have exactly the same coordinate differences,
all of them exact in the dtype too, so an evaluator that subtracts first gives the SAME BITS on the twin; one that scales first rounds
x * inv_ls at the magnitude of the offset and loses (offset / spread) eps.

Lattice.  x_i = 32 i, d = 1, inv_ls = 64, n = 600: every scaled distance is at least 2048, every off-diagonal value of all four kinds is exactly
0 in both dtypes, K = kappa I.  All residuals tie at every step of a pivoted Cholesky: the pivots are 0, 1, 2, ... only if the tie-break is
"lowest index" across the tiles as well as inside one.

Nearly flat.  gram_edge_cases' huge_lengthscale at d = 3, n = 300 (inv_ls = 2^-20): K is kappa 1 1^T to 1e-10 (smooth kinds), rank 1.
"""
import numpy as np

from tests import gram_edge_cases as E
from tests import nystrom_oracle as NO

KIND_NAME = {E.SE: "se", E.M12: "matern12", E.M32: "matern32", E.M52: "matern52"}
KINDS = tuple(KIND_NAME)
FAR_OFFSET = 1000
SHIFTS = ("offset", "offset_per_column", "offset_far")
LATTICE_N, LATTICE_M, LATTICE_KAPPA = 600, 300, 4.0
FLAT_N, FLAT_D = 300, 3
FLAT_TOL = {"f64": 1e-6, "f32": 1e-3}
FLAT_KINDS = (E.SE, E.M32, E.M52)          # Matern 1/2 leaves a second residual of 5e-6: no margin against the float64 tolerance


def ard_inv_ls(d, dt):
	"""The ARD vector of the module docstring for d coordinates, float64 array of dtype-representable values."""
	T = E.DTYPES[dt]
	rng = np.random.RandomState(9100 + 10 * d + (dt == "f32"))
	if d == 1:
		v = np.array([0.83])
	else:
		rung = np.arange(d) / (d - 1.0)
		jitter = np.where((rung > 0) & (rung < 1), rng.uniform(-0.2, 0.2, size=d) / (d - 1.0), 0.0)
		v = 0.31 * (1.45 / 0.31) ** (rung + jitter)
		while True:
			p = rng.permutation(d)
			if d == 2 or (np.any(np.diff(p) > 0) and np.any(np.diff(p) < 0)):
				break
		v = v[p]
	v = (v / np.sqrt(d)).astype(T).astype(np.float64)
	for _ in range(8):                                                    # (float64: a fixed point of x -> 1 / (1 / x); one step as a rule)
		w = (1.0 / (1.0 / v)).astype(T).astype(np.float64)
		if np.array_equal(w, v):
			break
		v = w
	assert np.array_equal((1.0 / (1.0 / v)).astype(T).astype(np.float64), v)
	assert np.array_equal(v.astype(T).astype(np.float64), v)
	assert not np.any(np.frexp(v)[0] == 0.5), "no power of two"
	s = np.sort(v)
	assert d == 1 or (s[-1] >= 4 * s[0] and np.all(s[1:] >= 1.01 * s[:-1]))
	v.setflags(write=False)
	return v


def gamma_of(case):
	"""Lengthscales for tests/nystrom_oracle.py, one per coordinate; 1 / gamma rounded to the dtype is the case's inv_ls again."""
	g = 1.0 / case.inv_ls
	assert np.array_equal((1.0 / g).astype(case.np_dtype).astype(np.float64), case.inv_ls)
	return g


def shift_vector(shift, d, dt):
	if shift == "offset_far":
		return np.full(d, float(FAR_OFFSET))
	assert shift in ("offset", "offset_per_column")
	return E._shift_vector(shift, d, dt)


def _exact(v, dt):
	return np.array_equal(v.astype(E.DTYPES[dt]).astype(np.float64), v)


def ard_case(layout, d, dt, n, q, same=False):
	"""A centred layout of gram_edge_cases (cube, duplicates) with the ARD vector in place of its own inverse lengthscales."""
	assert layout in ("cube", "duplicates")
	c = E.make_case(layout, d, dt, n, q, same)
	return E.Case(layout, d, dt, c.a, c.b, ard_inv_ls(d, dt), same)


def twin(case, shift):
	"""The translate of a case by integers: the same inv_ls, exactly the same coordinate differences.  Both members, and every difference
	of two coordinates of either, are exact in the dtype (asserted)."""
	s = shift_vector(shift, case.a.shape[1], case.dt)
	a = case.a + s
	b = a if case.same else case.b + s
	for v in (case.a, case.b, a, b):
		assert _exact(v, case.dt), "twin members must be exact in %s" % case.dt
	assert np.array_equal(a - s, case.a) and np.array_equal(b - s, case.b)
	lo, hi = min(case.a.min(), case.b.min()), max(case.a.max(), case.b.max())
	assert (hi - lo) * E.GRID[case.dt] < 2.0 ** (24 if case.dt == "f32" else 53), "differences must be exact in %s" % case.dt
	a.setflags(write=False); b.setflags(write=False)
	return E.Case(case.layout + "+" + shift, case.d, case.dt, a, b, case.inv_ls, case.same)


def wide_case(layout, d, dt, n, q, same=False, width=40):
	"""(the wide case, cols, the gathered case): d coordinates read as a shuffled, non-monotone subset of a ``width``-wide layout, with the ARD
	vector of d; the gathered case holds those columns contiguously.  The wide case's own inv_ls (one per stored column) is not used."""
	w = E.make_case(layout, width, dt, n, q, same)
	rng = np.random.RandomState(9300 + d)
	while True:
		cols = [int(c) for c in rng.permutation(width)[:d]]
		if np.any(np.diff(cols) > 0) and np.any(np.diff(cols) < 0):
			break
	return w, cols, E.sub_columns(w, cols, ard_inv_ls(d, dt))


DIMS = (1, 3, 7, 12, 20, 33)          # the register forms of kmv.hip (4, 8, 16 coordinates) and two and three rounds through LDS
SHAPES = ((129, 129, True), (70, 150, False))          # (n, q, a is b)


def entry_cases(d, dt, n, q, same):
	"""The layouts of the entry-by-entry tests as (name, case, name of the centred layout it is the twin of or None)."""
	out = []
	for layout in ("cube", "duplicates"):
		c = ard_case(layout, d, dt, n, q, same)
		out.append((layout, c, None))
		for shift in SHIFTS:
			if (shift == "offset_far" and dt == "f64") or (shift == "offset_per_column" and layout == "duplicates"):
				continue
			out.append((layout + "+" + shift, twin(c, shift), layout))
	for layout in ("clusters_offset", "tiny_lengthscale", "huge_lengthscale"):
		out.append((layout, E.make_case(layout, d, dt, n, q, same), None))
	return out


def discriminates(name, d, dt):
	"""Twins on which the scale-first order must miss the bound by a factor 2 (tests/test_direct_eval_cases_cpu.py asserts it): the
	error of that order is about (offset / lengthscale) eps per coordinate against a bound that grows with d, so float32 at offset 100
	separates the two orders only up to d = 3; the far twin does at every d."""
	if "+" not in name:
		return False
	shift = name.split("+")[1]
	if dt == "f64":
		return shift == "offset" or d <= 20
	return shift == "offset_far" or (shift == "offset" and d <= 3)


def lattice_case(dt):
	x = 32.0 * np.arange(LATTICE_N, dtype=np.float64).reshape(-1, 1)
	il = np.array([64.0])
	assert _exact(x, dt)
	x.setflags(write=False); il.setflags(write=False)
	return E.Case("lattice", 1, dt, x, x, il, True)


def flat_case(dt):
	return E.make_case("huge_lengthscale", FLAT_D, dt, FLAT_N, FLAT_N, True)


# ------------------------------------------------------------------------------------------------------------------------------
# the two orders of forming a scaled difference, in the dtype of the case (out[j][i] as in gram_edge_cases)
def emulate_r2(case, order):
	"""r^2 (q, n) in the dtype: "subtract_first" is (b - a) * il, what the contract states; "scale_first" is b * il - a * il, the form it
	rules out (E.emulate_r2(case, "direct"))."""
	if order == "scale_first":
		return E.emulate_r2(case, "direct")
	assert order == "subtract_first"
	T = case.np_dtype
	a, b, il = case.a.astype(T), case.b.astype(T), case.inv_ls.astype(T)
	r2 = np.zeros((case.q, case.n), dtype=T)
	for k in range(case.d):
		u = (b[:, k, None] - a[None, :, k]) * il[k]
		r2 += u * u
	return r2


def order_error(case, kind, order):
	"""max |phi(r2 of the order) - phi(r2 true)| at kappa = 1, phi in longdouble: the error of the distance alone."""
	r2t, _, _ = E.sq_dist_and_dot(case)
	return float(np.max(np.abs(E.phi_of_r2(kind, emulate_r2(case, order).astype(E.LD)) - E.phi_of_r2(kind, r2t))))


def oracle_kernel(case, kind, kappa=1.0, dtype=np.float64):
	"""tests/nystrom_oracle.kernel on the case with the per-coordinate lengthscales, laid out as the truth: out[j][i] = k(b_j, a_i)."""
	return NO.kernel(KIND_NAME[kind], case.b, case.a, gamma_of(case), kappa, dtype=dtype)
