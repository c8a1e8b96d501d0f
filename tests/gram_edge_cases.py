"""
Shared inputs, truth and error bounds for the Gram-kernel edge tests (tests/test_gram_edge_cases_cpu.py on the CPU,
tests/test_gpu_gram_edges.py through the C ABI).  Plain numpy, no GPU code.

Inputs.  Coordinates live on a dyadic grid in [-1, 1] (integers / 2^10 in fp32, integers / 2^30 in fp64); offsets are integers (1000
in fp64, 100 in fp32), so a translated layout is stored EXACTLY in its dtype (17 of 24 and 40 of 53 bits) and has exactly the pairwise
differences of the centred one.  The fp64 grid is the finer one on purpose: on a 2^-10 grid the squares and products of 1000 + k / 1024
need only 42 bits, the uncentred norm expansion would be EXACT in fp64, and a test on such points could not tell it from a robust one.  Off-centre layouts
use inverse lengthscales that are powers of two, so scaling is exact too and "scale then subtract" specifies the same value as
"subtract then scale".  Random inverse lengthscales in [0.3, 1.5] (rounded to the dtype) stay in the centred layouts.

Truth.  (b_j - a_i)[cols] * inv_ls in numpy.longdouble from the dtype-rounded inputs, then the closed forms of include/stpy_hip.h.

Bounds (derived from the number format, not from any kernel's output; eps = machine epsilon of the dtype):
  norm-expansion routes (SE always; Matern 3/2, 5/2 with a workspace)
      |K - K_true| <= kappa (c_kind 4 (d + 3) eps D^2 + 8 eps)
    D^2 the largest scaled squared distance between two points of a u b (the DIAMETER of the data), c_kind = max |d phi / d r^2|
    (1/2, 3/2, 5/6 for SE, Matern 3/2, 5/2): a (d + 3)-term expansion of r^2 about a point inside the data has every term below D^2,
    each rounded a few times; 8 eps covers the evaluation of phi (exp to 2 ulp, fp32 __expf's |t| e^t eps <= 0.37 eps, prefactors).
  direct-difference routes (Matern 1/2 always; Matern 3/2, 5/2 without a workspace)
      |K - K_true| <= kappa (d + 8) eps          (r to (d + 2) / 2 eps relative, |r phi'(r)| < 1, the rest for phi itself)
  LINEAR: (d + 2) eps sum_k |a_k b_k| on the inner product (times kappa, + 2 eps |K_true| for the scale and the offset);
  POLY degree p: the same delta on s = <a, b> + offset through the power, p (|s| + delta)^(p - 1) delta (mean-value form, so it holds
    when s is near zero), + (p + 2) eps |K_true| for the p roundings of the repeated product and the scale, + the smallest normal
    number (a power of |s| < 1 may underflow on the way).
"""
import functools

import numpy as np

LD = np.longdouble
GRID = {"f64": 2 ** 30, "f32": 2 ** 10}
SE, M12, M32, M52, LIN, POLY = 0, 1, 2, 3, 4, 5
STATIONARY = (SE, M12, M32, M52)
POLY_DEGREES = (1, 2, 3, 7, 64)
DIMS = (1, 3, 16, 33)
DTYPES = {"f64": np.float64, "f32": np.float32}
OFFSET = {"f64": 1000, "f32": 100}
LAYOUTS = ("cube", "offset", "offset_per_column", "duplicates", "duplicates_offset", "clusters", "clusters_offset",
           "tiny_lengthscale", "huge_lengthscale")
OFFSET_LAYOUTS = ("offset", "offset_per_column")
C_KIND = {SE: 0.5, M32: 1.5, M52: 5.0 / 6.0}
N_DUP, N_NEAR = 12, 6
# tiny_lengthscale (inv_ls = 64): coordinate gaps along the first axis that put the exponent of each family into the band where
# the result is a denormal of the dtype, and one below the clamp / the smallest denormal.  Exponents: SE -2048 g^2, Matern 1/2
# -64 g, 3/2 and 5/2 -64 sqrt(3 | 5) g plus the log of the polynomial prefactor; fp64 band [-745, -708], fp32 band about [-103, -87.4].  All gaps are dyadic.
TINY_GAPS = {
	"f64": (605 / 1024, 610 / 1024, 615 / 1024, 11.25, 6.5, 5.125, 13.0, 0.75),
	"f32": (214 / 1024, 220 / 1024, 228 / 1024, 1.5, 0.85009765625, 0.6875, 2.0, 0.3125),
}


def eps_of(dt):
	return float(np.finfo(DTYPES[dt]).eps)


class Case(object):
	"""a: (n, d), b: (q, d) float64 arrays that hold dtype-representable values; inv_ls likewise; same: b is a."""
	def __init__(self, layout, d, dt, a, b, inv_ls, same):
		self.layout, self.d, self.dt, self.a, self.b, self.inv_ls, self.same = layout, d, dt, a, b, inv_ls, same
		self.n, self.q = a.shape[0], b.shape[0]
		self.eps = eps_of(dt)
		self._memo = {}

	@property
	def np_dtype(self):
		return DTYPES[self.dt]


def _pow2_inv_ls(d):
	"""Powers of two mixed per column, 0.25 .. 2 at d = 1 and scaled down by about sqrt(d) (lengthscales near sqrt(d), as everywhere in
	the suite: with shorter ones almost every pair of a d = 33 layout sits where the kernel is flat and no distance error shows)."""
	scale = 2.0 ** -(int(np.log2(d)) // 2)
	return np.array([(0.25, 0.5, 1.0, 2.0)[k % 4] for k in range(d)]) * scale


def _shift_vector(layout, d, dt):
	c = OFFSET[dt]
	if layout in ("offset", "duplicates_offset", "clusters_offset"):
		return np.full(d, float(c))
	if layout == "offset_per_column":
		return np.array([float(round(c * (k + 1) / d)) for k in range(d)])
	return np.zeros(d)


@functools.lru_cache(maxsize=None)
def make_case(layout, d, dt, n, q, same=False):
	"""The inputs of one layout.  Deterministic in its arguments."""
	assert layout in LAYOUTS and dt in DTYPES
	rng = np.random.RandomState(1000 * LAYOUTS.index(layout) + 10 * d + (dt == "f32") + 7 * n + 3 * q)
	grid = GRID[dt]
	a = rng.randint(-grid, grid + 1, size=(n, d)) / float(grid)
	b = a if same else rng.randint(-grid, grid + 1, size=(q, d)) / float(grid)
	if layout in ("cube", "duplicates"):
		inv_ls = rng.uniform(0.3, 1.5, size=d).astype(DTYPES[dt]).astype(np.float64)
	elif layout in ("clusters", "clusters_offset"):
		inv_ls = np.full(d, 0.25)
	elif layout == "tiny_lengthscale":
		inv_ls = np.full(d, 64.0)
	elif layout == "huge_lengthscale":
		inv_ls = np.full(d, 2.0 ** -20)
	else:
		inv_ls = _pow2_inv_ls(d)
	step = 1.0 / grid
	if layout in ("duplicates", "duplicates_offset"):
		# exact copies of rows of a, and pairs one grid step apart in one coordinate
		if same:
			h = n // 2
			a[h:h + N_DUP] = a[:N_DUP]
			for i in range(N_NEAR):
				a[h + N_DUP + i] = a[N_DUP + i]
				a[h + N_DUP + i, i % d] += step
		else:
			b[3:3 + N_DUP] = a[:N_DUP]
			for i in range(N_NEAR):
				b[3 + N_DUP + i] = a[N_DUP + i]
				b[3 + N_DUP + i, i % d] += step
	if layout in ("clusters", "clusters_offset"):
		a[1::2] += 40.0                       # (in place: with same, b is a)
		if not same:
			b[::2] += 40.0
	if layout == "tiny_lengthscale":
		gaps = TINY_GAPS[dt]
		if same:
			h = n // 2
			for i, g in enumerate(gaps):
				a[h + i] = a[i]
				a[h + i, 0] += g
			a[h + len(gaps)] = a[len(gaps)]                      # and one exact copy
		else:
			for i, g in enumerate(gaps):
				b[5 + i] = a[i]
				b[5 + i, 0] += g
			b[5 + len(gaps)] = a[len(gaps)]
	shift = _shift_vector(layout, d, dt)
	a += shift
	if not same:
		b += shift
	for v in (a, b, inv_ls):
		assert np.array_equal(v.astype(DTYPES[dt]).astype(np.float64), v), "case inputs must be exact in %s" % dt
	a.setflags(write=False); b.setflags(write=False); inv_ls.setflags(write=False)
	return Case(layout, d, dt, a, b, inv_ls, same)


def sub_columns(case, cols, inv_ls=None):
	"""The case restricted to a column subset (what a kernel with `cols` sees); inv_ls: per selected column (default: the case's)."""
	cols = list(cols)
	il = case.inv_ls[cols] if inv_ls is None else np.asarray(inv_ls, dtype=np.float64)
	a = np.ascontiguousarray(case.a[:, cols])
	return Case(case.layout, len(cols), case.dt, a, a if case.same else np.ascontiguousarray(case.b[:, cols]), il, case.same)


def sq_dist_and_dot(case):
	"""(r^2, <b_j, a_i>, sum_k |b_jk a_ik|) of the scaled points, (q, n) longdouble; r^2 from direct differences."""
	if "sq" not in case._memo:
		case._memo["sq"] = _sq_dist_and_dot(case)
	return case._memo["sq"]


def _sq_dist_and_dot(case):
	a, b, il = case.a.astype(LD), case.b.astype(LD), case.inv_ls.astype(LD)
	r2 = np.zeros((case.q, case.n), dtype=LD)
	dot = np.zeros_like(r2)
	adot = np.zeros_like(r2)
	for k in range(case.d):
		u = (b[:, k, None] - a[None, :, k]) * il[k]
		r2 += u * u
		p = (b[:, k, None] * il[k]) * (a[None, :, k] * il[k])
		dot += p
		adot += np.abs(p)
	return r2, dot, adot


def phi_of_r2(kind, r2):
	"""The stationary closed forms of include/stpy_hip.h on a squared scaled distance, in the precision of r2."""
	r2 = np.asarray(r2)
	one = r2.dtype.type(1)
	if kind == SE:
		return np.exp(-r2 / 2)
	r = np.sqrt(r2)
	if kind == M12:
		return np.exp(-r)
	if kind == M32:
		t = r * np.sqrt(r2.dtype.type(3))
		return (one + t) * np.exp(-t)
	if kind == M52:
		t = r * np.sqrt(r2.dtype.type(5))
		return (one + t + t * t / 3) * np.exp(-t)
	raise ValueError(kind)


def truth_ld(case, kind, kappa=1.0, offset=0.0, degree=0):
	"""kappa phi(...) (+ offset for LINEAR) in longdouble, (q, n): out[j][i] = k(b_j, a_i)."""
	r2, dot, _ = sq_dist_and_dot(case)
	if kind in STATIONARY:
		return LD(kappa) * phi_of_r2(kind, r2)
	if kind == LIN:
		return LD(kappa) * dot + LD(offset)
	if kind == POLY:
		return LD(kappa) * (dot + LD(offset)) ** int(degree)
	raise ValueError(kind)


def truth(case, kind, kappa=1.0, offset=0.0, degree=0):
	with np.errstate(over="ignore"):
		return truth_ld(case, kind, kappa, offset, degree).astype(np.float64)


def diameter_sq(case):
	"""Largest scaled squared distance between any two points of a u b."""
	if "D2" not in case._memo:
		case._memo["D2"] = _diameter_sq(case)
	return case._memo["D2"]


def _diameter_sq(case):
	pts = case.a if case.same else np.concatenate([case.a, case.b], axis=0)
	xs = (pts - pts[0]) * case.inv_ls                      # (exact shift on these inputs; only the differences matter)
	nrm = np.sum(xs * xs, axis=1)
	best = 0.0
	for s in range(0, xs.shape[0], 512):
		blk = nrm[s:s + 512, None] + nrm[None, :] - 2.0 * xs[s:s + 512] @ xs.T
		best = max(best, float(blk.max()))
	return best * (1.0 + 1e-12)


def expansion_bound(case, kind, kappa=1.0, c_kind=None):
	c = C_KIND[kind] if c_kind is None else c_kind
	return abs(kappa) * (c * 4.0 * (case.d + 3) * case.eps * diameter_sq(case) + 8.0 * case.eps)


def direct_bound(case, kappa=1.0):
	return abs(kappa) * (case.d + 8) * case.eps


def stationary_bound(case, kind, workspace, kappa=1.0):
	"""The bound of the route that serves a stationary kind: norm expansion for SE and, with a workspace, Matern 3/2 and 5/2."""
	if kind == SE or (workspace and kind in (M32, M52)):
		return expansion_bound(case, kind, kappa)
	return direct_bound(case, kappa)


def dot_kind_bound(case, kind, kappa=1.0, offset=0.0, degree=0):
	"""Elementwise bound (q, n) longdouble for LINEAR / POLY, see the module docstring."""
	_, dot, adot = sq_dist_and_dot(case)
	eps = LD(case.eps)
	delta = (case.d + 2) * eps * adot + eps * abs(LD(offset))
	if kind == LIN:
		return abs(LD(kappa)) * delta + 2 * eps * np.abs(LD(kappa) * dot + LD(offset)) + eps * abs(LD(offset))
	p = int(degree)
	s = np.abs(dot + LD(offset))
	return abs(LD(kappa)) * (p * (s + delta) ** (p - 1) * delta + (p + 2) * eps * s ** p + LD(np.finfo(case.np_dtype).tiny))


# ------------------------------------------------------------------------------------------------------------------------------
# numpy emulations of the three ways of forming r^2, in the dtype of the case (phi is then applied in longdouble, so what is
# measured is the error of the distance alone: the 8 eps term of the bound stays as room for phi on the device)
def emulate_r2(case, how):
	T = case.np_dtype
	a, b, il = case.a.astype(T), case.b.astype(T), case.inv_ls.astype(T)
	if how == "direct":
		r2 = np.zeros((case.q, case.n), dtype=T)
		for k in range(case.d):
			u = b[:, k, None] * il[k] - a[None, :, k] * il[k]
			r2 += u * u
		return r2
	if how == "shifted":
		ref = a[0].copy()
		a, b = a - ref, b - ref
	elif how != "raw":
		raise ValueError(how)
	xa, xb = a * il, b * il
	na = np.zeros(case.n, dtype=T)
	nb = np.zeros(case.q, dtype=T)
	acc = np.zeros((case.q, case.n), dtype=T)
	for k in range(case.d):                 # sequential accumulation in the dtype, as the kernels do
		na += xa[:, k] * xa[:, k]
		nb += xb[:, k] * xb[:, k]
		acc += xb[:, k, None] * xa[None, :, k]
	return nb[:, None] + na[None, :] - T(2) * acc


def emulated_error(case, kind, how):
	"""max |phi(r2_emulated) - phi(r2_true)| (kappa = 1); negative r^2 is clamped for the Matern forms as the kernels do."""
	r2 = emulate_r2(case, how).astype(LD)
	if kind != SE:
		r2 = np.maximum(r2, LD(0))
	r2t, _, _ = sq_dist_and_dot(case)
	return float(np.max(np.abs(phi_of_r2(kind, r2) - phi_of_r2(kind, r2t))))


# ------------------------------------------------------------------------------------------------------------------------------
# evidence-gradient weights: F of d k / d lengthscale_m = kappa F u_m^2 / lengthscale_m (include/stpy_hip.h, stpy_lml_weight)
def dfactor_of_r2(kind, r2):
	"""F per family on a squared scaled distance; Matern 1/2 is exp(-r) / r (inf at r = 0: the caller masks coincident pairs)."""
	r2 = np.asarray(r2)
	one = r2.dtype.type(1)
	if kind == SE:
		return np.exp(-r2 / 2)
	r = np.sqrt(r2)
	if kind == M12:
		with np.errstate(divide="ignore", invalid="ignore"):
			return np.exp(-r) / r
	if kind == M32:
		return 3 * np.exp(-r * np.sqrt(r2.dtype.type(3)))
	if kind == M52:
		t = r * np.sqrt(r2.dtype.type(5))
		return (one + t) * np.exp(-t) * 5 / 3
	raise ValueError(kind)
