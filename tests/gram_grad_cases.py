"""
Cases, oracle and error bounds for stpy_gram_grad (csrc/grad.hip): tests/test_gram_grad_cases_cpu.py shows on the CPU that they tell a right
evaluator from a wrong one, tests/test_gpu_gram_grad_edges.py runs them through the C ABI.  Plain numpy, no GPU code, no library.  Built on
tests/gram_edge_cases.py (grids, offsets, layouts, make_case) and tests/direct_eval_cases.py (ard_inv_ls, twin, wide_case).

The operation (include/stpy_hip.h).  e_tik = (xt_t - x_i)[cols[k]] * inv_ls[k], c_ti = u_t alpha_i + v_t Wt[t, i] (a NULL scale is 1),
    G[t, cols[k]]          (op)= inv_ls[k]           sum_i c_ti psi_ti e_tik
    H[t, cols[k], cols[l]] (op)= inv_ls[k] inv_ls[l] sum_i c_ti (chi_ti e_tik e_til + [k == l] psi_ti)
with psi = kappa phi'(r) / r and chi = psi'(r) / r of the family (r^2 = sum_k e_k^2):
    SE          psi = -kappa exp(-r^2 / 2)                             chi = kappa exp(-r^2 / 2)
    Matern 1/2  psi = -kappa exp(-r) / r, and 0 at r = 0: a coincident pair contributes exactly zero            (no Hessian)
    Matern 3/2  psi = -3 kappa exp(-sqrt(3) r)                                                                  (no Hessian)
    Matern 5/2  psi = -(5 / 3) kappa (1 + sqrt(5) r) exp(-sqrt(5) r)   chi = (25 / 3) kappa exp(-sqrt(5) r)
The two dot-product kinds differentiate kappa phi(b), b = sum_k (xt_k inv_ls_k)(x_ik inv_ls_k) + offset: the factor e_tik is the scaled
training coordinate x_ik inv_ls_k alone, there is no [k == l] term, and psi = kappa, chi = 0 (LINEAR), psi = kappa p b^(p - 1),
chi = kappa p (p - 1) b^(p - 2) (POLY of degree p).  kappa and offset of every case are exact in float32.

Oracle.  All of the above in numpy.longdouble from the dtype-rounded inputs (the cases hold float64 arrays of dtype-exact values).

Bound.  Entry by entry |G - G_true|[t, k] <= c eps S_tk, S_tk = inv_ls_k sum_i |c_ti psi_ti e_tik| the sum of the absolute values of
the terms (the Hessian the same with its own S, the sum of |c chi e_k e_l| and, on the diagonal, |c psi|).  eps is the machine epsilon
of the dtype, one rounding is eps / 2.  c is counted from the number format and the kernel's plan, never from the kernel's output:
  one term, c_term = 4 + c_psi (relative to the term)
      coefficient 2.5   fl(u alpha) and one fma: (|u alpha| + |c|) eps / 2, and the cases keep |u alpha| + |v Wt| <= 4 |c| (asserted)
      e_k         1     the difference and its scaling, one rounding each (per factor e: 2 in the e_k e_l terms of the Hessian); the
                        kernel may apply the scaling of the gradient's factor after the sum instead, the count is the same
      c psi       0.5   (the product with e_k is rounded inside the accumulating fma: counted with the sum)
      c_psi = 6 + (d + 5) / 2 * lam + 2.5 |t|, per pair and inside the sum, since it grows with the pair's distance:
          r^2 is d squares of factors with 2 roundings each, summed by fma: (d + 5) eps / 2 relative (no more if ONE lengthscale is
          applied to the sum of the squared raw differences: one rounding per factor and two for inv_ls^2);  lam = |d log psi / d log r^2| is
          r^2 / 2 (SE), (r + 1) / 2 (Matern 1/2), sqrt(3) r / 2 (3/2), 5 r^2 / (2 (1 + sqrt(5) r)) (5/2; sqrt(5) r / 2 for chi);
          t is the argument of exp: up to three roundings on the way to it (sqrt, the constant, their product) move the result by
          1.5 |t| eps, an exp whose error grows with its argument (the hardware's exp2 behind a scaling) by |t| eps more;
          6: exp itself to 2 ulp (2 eps, as tests/gram_edge_cases.py grants) and up to 8 roundings in the prefactors (Matern 5/2).
      POLY has no exp: the inner product is off by delta_b = (d + 2) eps sum_k |a_k b_k| + eps |offset| (the bound of
          tests/gram_edge_cases.py), psi by kappa p (p - 1) (|b| + delta_b)^(p - 2) delta_b absolutely (mean-value form, chi alike one
          degree lower), and the repeated product and its two scales add (p + 2) eps / 2 relative.
      Every psi, chi and c psi may also underflow: the smallest normal number of the dtype, absolutely, each.
  the fixed-order sum, c_sum = (L + 15 + 15 + nsplit) / 2: a lane adds L = ceil(chunk / 256) terms in sequence (one fma each; the
      Hessian's diagonal adds two numbers per term: 2 L), then the 16-lane rows and the 16 row sums of the workgroup tree, then the
      nsplit chunk sums: at most that many roundings lie between a term and the result, each relative to a partial sum that the sum of
      absolute values bounds.  chunk and nsplit are those of grad_plan (csrc/grad.hip), mirrored in plan() below.
  the final factor inv_ls_k: 0.5 (the Hessian: 1, inv_ls_k inv_ls_l and its product with the sum).
The analysis is first order; c eps stays below 1e-3 in both dtypes (asserted), and the bound is multiplied by 1.001 for the rest.
Absolute floor: tiny (inv_ls_k sum_i (|c e_k| + |e_k|) + 1), tiny the smallest normal number -- the underflows named above, which decide
only on the tiny-lengthscale layouts.  Under ADD the result is fl(G0 + sum): eps / 2 of |G0 + G_true| more.

Twins.  A centred layout (cube, duplicates) with ARD inverse lengthscales that are no powers of two (cube_iso: one such value in every
coordinate, which the kernel serves by a distance loop of its own), and its translates by integers
(tests/direct_eval_cases.py: offset, offset_per_column, and for float32 offset_far): all coordinate differences are the same and
exact, so a kernel that subtracts before it scales returns the SAME BITS on the twin.  One that scales first rounds x * inv_ls at the
magnitude of the offset and loses (offset / spread) eps.
"""
import zlib

import numpy as np

from tests import direct_eval_cases as D
from tests import gram_edge_cases as E

LD = E.LD
GG_THREADS, GG_TM, GG_QB, GG_TARGET_WGS = 256, 4, 16, 2048          # csrc/grad.hip
SENTINEL = -7.25
SET, ADD = 0, 1

# name -> (kind, degree, kappa, offset); kappa and offset exact in float32
FAMILIES = dict([("se", (E.SE, 0, 1.5, 0.0)), ("m12", (E.M12, 0, 1.25, 0.0)), ("m32", (E.M32, 0, 0.75, 0.0)), ("m52", (E.M52, 0, 1.5, 0.0)),
                 ("lin", (E.LIN, 0, 1.25, 0.25))] + [("poly%d" % p, (E.POLY, p, 0.5, 1.0)) for p in E.POLY_DEGREES])
STATIONARY_FAMILIES = ("se", "m12", "m32", "m52")
HESSIAN_FAMILIES = tuple(f for f in FAMILIES if f not in ("m12", "m32"))
FAMILY_GROUP = {f: (f if f in STATIONARY_FAMILIES or f == "lin" else "poly") for f in FAMILIES}          # the six families
COEF_FORMS = ("both", "both_noscale", "alpha_u", "alpha", "wt_v", "wt")


def plan(m, n, d, order):
	"""grad_plan of csrc/grad.hip: (Q, nqb, chunk, nsplit, ntiles)."""
	Q = d + (d * d if order == 2 else 0)
	nqb = (Q + GG_QB - 1) // GG_QB
	ntiles = (m + GG_TM - 1) // GG_TM
	base = nqb * ntiles
	want = (GG_TARGET_WGS + base - 1) // base
	want = max(1, min(want, (n + GG_THREADS - 1) // GG_THREADS))
	chunk = (n + want - 1) // want
	chunk = (chunk + GG_THREADS - 1) // GG_THREADS * GG_THREADS
	return Q, nqb, chunk, (n + chunk - 1) // chunk, ntiles


class GradCase(object):
	"""One call of stpy_gram_grad.  x (n, ldx), xt (m, ldt), inv_ls (d,), alpha (n,), u / v (m,), Wt (m, ldw), G0 (m, ldg), H0 (m, ldg, ldg):
	float64 arrays of dtype-exact values (or None); cols: list of d column indices or None; twin_of: the name of the centred case whose
	bits this one must reproduce."""
	def __init__(self, name, family, dt, x, xt, inv_ls, cols=None, order=1, form="both", combine=SET, ldg=None, twin_of=None, coef_key=None):
		self.name, self.family, self.dt, self.order, self.form, self.combine, self.twin_of = name, family, dt, order, form, combine, twin_of
		self.kind, self.degree, self.kappa, self.offset = FAMILIES[family]
		self.x, self.xt, self.inv_ls, self.cols = x, xt, np.asarray(inv_ls, dtype=np.float64), (None if cols is None else list(cols))
		self.n, self.m, self.d = x.shape[0], xt.shape[0], len(self.inv_ls)
		self.sel = list(range(self.d)) if cols is None else self.cols
		assert len(self.sel) == self.d == len(set(self.sel)) and max(self.sel) < min(x.shape[1], xt.shape[1])
		self.ldg = (self.d if cols is None else max(self.sel) + 1) if ldg is None else ldg
		assert self.ldg > max(self.sel)
		assert order == 1 or family in HESSIAN_FAMILIES
		self.eps = E.eps_of(dt)
		self.tiny = float(np.finfo(E.DTYPES[dt]).tiny)
		self.dot = self.kind in (E.LIN, E.POLY)
		self._coefficients(coef_key or name)
		self._memo = {}

	@property
	def np_dtype(self):
		return E.DTYPES[self.dt]

	def _coefficients(self, key):
		"""Standard normal draws rounded to the dtype, seeded by `key` (a twin shares its centred case's).  ldw = n + 5.  Where both halves
		are present, Wt changes sign on the pairs where u alpha and v Wt cancel to less than a quarter of their magnitudes: the bound is
		relative to |c|.  ADD: random initial contents; SET: the sentinel."""
		T = self.np_dtype
		rng = np.random.RandomState(zlib.crc32(("%s/%s/%s" % (key, self.dt, self.form)).encode()) & 0x7fffffff)
		r = lambda *shape: rng.standard_normal(shape).astype(T).astype(np.float64)
		n, m = self.n, self.m
		alpha, u, Wt, v = r(n), r(m), r(m, n + 5), r(m)
		form = self.form
		assert form in COEF_FORMS
		self.alpha = alpha if form in ("both", "both_noscale", "alpha_u", "alpha") else None
		self.u = u if form in ("both", "alpha_u") else None
		self.Wt = Wt if form in ("both", "both_noscale", "wt_v", "wt") else None
		self.v = v if form in ("both", "wt_v") else None
		if self.alpha is not None and self.Wt is not None:
			pa = (1.0 if self.u is None else self.u[:, None]) * self.alpha[None, :]
			pw = (1.0 if self.v is None else self.v[:, None]) * self.Wt[:, :n]
			flip = np.abs(pa + pw) * 4 < np.abs(pa) + np.abs(pw)
			self.Wt[:, :n][flip] *= -1.0
			pw = (1.0 if self.v is None else self.v[:, None]) * self.Wt[:, :n]
			assert np.all(np.abs(pa) + np.abs(pw) <= 4 * np.abs(pa + pw))
		if self.combine == ADD:
			self.G0, self.H0 = r(m, self.ldg), (r(m, self.ldg, self.ldg) if self.order == 2 else None)
		else:
			self.G0 = np.full((m, self.ldg), SENTINEL)
			self.H0 = np.full((m, self.ldg, self.ldg), SENTINEL) if self.order == 2 else None

	def coef_ld(self):
		"""c_ti in longdouble, (m, n)."""
		c = np.zeros((self.m, self.n), dtype=LD)
		if self.alpha is not None:
			c = c + (LD(1) if self.u is None else self.u.astype(LD)[:, None]) * self.alpha.astype(LD)[None, :]
		if self.Wt is not None:
			c = c + (LD(1) if self.v is None else self.v.astype(LD)[:, None]) * self.Wt[:, :self.n].astype(LD)
		return c


# ------------------------------------------------------------------------------------------------------------------------------
# oracle and bounds
def _pair_ld(gc):
	"""Per pair, in longdouble: the factors e_k (list of (m, n) or (1, n) arrays), psi, chi, and the error model of psi and chi
	(relative parts rpsi / rchi in units of eps, absolute parts apsi / achi)."""
	il = gc.inv_ls.astype(LD)
	x, xt = gc.x[:, gc.sel].astype(LD), gc.xt[:, gc.sel].astype(LD)
	d, eps, kappa = gc.d, LD(gc.eps), LD(gc.kappa)
	zero = np.zeros((gc.m, gc.n), dtype=LD)
	if not gc.dot:
		e = [(xt[:, k, None] - x[None, :, k]) * il[k] for k in range(d)]
		s = zero.copy()
		for ek in e:
			s = s + ek * ek
		r = np.sqrt(s)
		ds = LD(d + 5) / 2
		if gc.kind == E.SE:
			ex = np.exp(-s / 2)
			psi, chi, t = -kappa * ex, kappa * ex, s / 2
			lam_p = lam_c = s / 2
		elif gc.kind == E.M12:
			with np.errstate(divide="ignore", invalid="ignore"):
				psi = np.where(r > 0, -kappa * np.exp(-r) / np.where(r > 0, r, 1), LD(0))
			chi, t, lam_p, lam_c = zero, r, (r + 1) / 2, zero
		elif gc.kind == E.M32:
			t = np.sqrt(LD(3)) * r
			psi, chi, lam_p, lam_c = -3 * kappa * np.exp(-t), zero, t / 2, zero
		else:
			t = np.sqrt(LD(5)) * r
			ex = np.exp(-t)
			psi, chi = -(LD(5) / 3) * kappa * (1 + t) * ex, (LD(25) / 3) * kappa * ex
			lam_p, lam_c = 5 * s / (2 * (1 + t)), t / 2
		rpsi, rchi = 6 + ds * lam_p + LD(2.5) * t, 6 + ds * lam_c + LD(2.5) * t
		apsi = achi = zero + LD(gc.tiny)
		return e, psi, chi, rpsi, rchi, apsi, achi
	e = [(x[None, :, k] * il[k]) for k in range(d)]
	if gc.kind == E.LIN:
		return e, zero + kappa, zero, zero, zero, zero, zero
	p = gc.degree
	b, ab = zero + LD(gc.offset), zero.copy()
	for k in range(d):
		pr = (xt[:, k, None] * il[k]) * e[k]
		b, ab = b + pr, ab + np.abs(pr)
	delta = (d + 2) * eps * ab + eps * abs(LD(gc.offset))
	psi = kappa * p * b ** (p - 1)
	chi = kappa * p * (p - 1) * b ** (p - 2) if p >= 2 else zero
	apsi = (kappa * p * (p - 1) * (np.abs(b) + delta) ** (p - 2) * delta if p >= 2 else zero) + LD(gc.tiny)
	achi = (kappa * p * (p - 1) * (p - 2) * (np.abs(b) + delta) ** (p - 3) * delta if p >= 3 else zero) + LD(gc.tiny)
	rel = zero + LD(p + 2) / 2
	return e, psi, chi, rel, rel, apsi, achi


def oracle(gc):
	"""dict(G (m, d), bG, S_G, and for order 2 H (m, d, d), bH, S_H): the longdouble truth of the sums (without any initial contents), the
	entrywise bounds and the sums of absolute values, in the order of cols."""
	if "oracle" in gc._memo:
		return gc._memo["oracle"]
	e, psi, chi, rpsi, rchi, apsi, achi = _pair_ld(gc)
	il, eps, tiny = gc.inv_ls.astype(LD), LD(gc.eps), LD(gc.tiny)
	c = gc.coef_ld()
	ac = np.abs(c)
	_, _, chunk, nsplit, _ = plan(gc.m, gc.n, gc.d, gc.order)
	lane = (chunk + GG_THREADS - 1) // GG_THREADS
	m, d = gc.m, gc.d
	out = {}
	c_sum = LD(lane + 30 + nsplit) / 2
	c_fix = LD(4) + c_sum + LD(0.5)
	w1, aw1 = c * psi, ac * (eps * np.abs(psi) * (c_fix + rpsi) + apsi)
	G, bG, SG, rG = (np.zeros((m, d), dtype=LD) for _ in range(4))
	for k in range(d):
		ae = np.abs(e[k])
		G[:, k] = il[k] * np.sum(w1 * e[k], axis=1)
		SG[:, k] = il[k] * np.sum(np.abs(w1) * ae, axis=1)
		rG[:, k] = LD(1.001) * il[k] * np.sum(aw1 * ae, axis=1)
		bG[:, k] = rG[:, k] + tiny * (il[k] * np.sum((ac + 1) * ae, axis=1) + 1)
	live = np.abs(psi) >= tiny                        # (a pair whose psi has underflowed is left to the floor)
	out.update(G=G, bG=bG, S_G=SG, rel_G=rG, c_max=float(np.max(np.where(live, c_fix + rpsi, 0))))
	if gc.order == 2:
		c_sum = LD(2 * lane + 30 + nsplit) / 2
		c_fix = LD(5) + c_sum + LD(1)                     # (one more factor e than the gradient's terms)
		w2, aw2 = c * chi, ac * (eps * np.abs(chi) * (c_fix + rchi) + achi)
		aw1 = ac * (eps * np.abs(psi) * (c_fix + rpsi) + apsi)
		H, bH, SH, rH = (np.zeros((m, d, d), dtype=LD) for _ in range(4))
		for k in range(d):
			for l in range(k + 1):
				ee = e[k] * e[l]
				aee = np.abs(ee)
				h, sh, bh = np.sum(w2 * ee, axis=1), np.sum(np.abs(w2) * aee, axis=1), np.sum(aw2 * aee, axis=1)
				fl = np.sum((ac + 1) * aee, axis=1)
				if k == l and not gc.dot:
					h, sh, bh, fl = h + np.sum(w1, axis=1), sh + np.sum(np.abs(w1), axis=1), bh + np.sum(aw1, axis=1), fl + np.sum(ac + 1, axis=1)
				f = il[k] * il[l]
				H[:, k, l] = H[:, l, k] = f * h
				SH[:, k, l] = SH[:, l, k] = f * sh
				rH[:, k, l] = rH[:, l, k] = LD(1.001) * f * bh
				bH[:, k, l] = bH[:, l, k] = rH[:, k, l] + tiny * (f * fl + 1)
		out.update(H=H, bH=bH, S_H=SH, rel_H=rH, c_max=max(out["c_max"], float(np.max(np.where(live, c_fix + np.maximum(rpsi, rchi), 0)))))
	finite = [k for k in ("G", "bG", "H", "bH") if k in out]
	fmax = LD(np.finfo(gc.np_dtype).max)
	for k in finite:
		assert np.all(np.isfinite(out[k])) and np.all(np.abs(out[k]) < fmax / 16), (gc.name, k, "not representable in %s" % gc.dt)
	assert out["c_max"] * gc.eps < 1e-3, (gc.name, out["c_max"])
	gc._memo["oracle"] = out
	return out


def c_effective(gc):
	"""The largest (bound without its floor) / (eps S) over the entries: the `c` of the module docstring as it comes out on the case."""
	o = oracle(gc)
	best = 0.0
	for b, s in (("rel_G", "S_G"), ("rel_H", "S_H")):
		pos = o[s] * LD(gc.eps) > 1e6 * gc.tiny if b in o else None          # (below that the underflow terms take over)
		if pos is not None and pos.any():
			best = max(best, float(np.max(o[b][pos] / (LD(gc.eps) * o[s][pos]))))
	return best


# ------------------------------------------------------------------------------------------------------------------------------
# what a call has to leave in G and H
def gather(gc, Gbuf, Hbuf):
	"""The entries of the output buffers that the call owns, in the order of cols: (m, d) and (m, d, d) or None."""
	sel = gc.sel
	return Gbuf[:, sel], (None if Hbuf is None else Hbuf[:, sel][:, :, sel])


def check(gc, Gbuf, Hbuf):
	"""Compare the output buffers of a call ((m, ldg) and (m, ldg, ldg), in the dtype) with the oracle.  Returns dict(ratio_G, ratio_H: the
	largest error / bound, inf where an owned entry is NaN or Inf; untouched: every entry the call does not own has the bits it started
	with; exact_zero_G / exact_zero_offdiag_H: as named, for the coincident single-pair cases)."""
	o = oracle(gc)
	T = gc.np_dtype
	assert Gbuf.dtype == T and Gbuf.shape == (gc.m, gc.ldg)
	g, h = gather(gc, Gbuf, Hbuf)
	g0, h0 = gather(gc, gc.G0.astype(T), None if gc.H0 is None else gc.H0.astype(T))
	res = {}

	def ratio(got, start, true, bound):
		want = true + (start.astype(LD) if gc.combine == ADD else 0)
		bnd = bound + ((LD(gc.eps) / 2) * (np.abs(want) + bound) if gc.combine == ADD else 0)
		with np.errstate(invalid="ignore", divide="ignore"):
			q = np.abs(got.astype(LD) - want) / bnd
		q = np.where(np.isfinite(got) & ~np.isnan(q), q, np.inf)
		return float(np.max(q))
	res["ratio_G"] = ratio(g, g0, o["G"], o["bG"])
	own = np.zeros((gc.m, gc.ldg), dtype=bool)
	own[:, gc.sel] = True
	res["untouched"] = bool(np.array_equal(Gbuf[~own], gc.G0.astype(T)[~own]))
	res["exact_zero_G"] = bool(np.all(g == 0))
	if gc.order == 2:
		assert Hbuf.dtype == T and Hbuf.shape == (gc.m, gc.ldg, gc.ldg)
		res["ratio_H"] = ratio(h, h0, o["H"], o["bH"])
		ownh = own[:, :, None] & own[:, None, :]
		res["untouched"] = res["untouched"] and bool(np.array_equal(Hbuf[~ownh], gc.H0.astype(T)[~ownh]))
		res["exact_zero_offdiag_H"] = bool(np.all(h[:, ~np.eye(gc.d, dtype=bool)] == 0))
	else:
		res["ratio_H"] = 0.0
	res["ratio"] = max(res["ratio_G"], res["ratio_H"])
	return res


# ------------------------------------------------------------------------------------------------------------------------------
# a numpy evaluator in the dtype: per-pair arithmetic in the dtype, sums in a wider type; `plant` puts one named error into it
PLANTS = ("scale_first", "norm_expansion", "m12_unguarded", "inv_ls_by_col", "no_w1_diag", "no_final_scale", "swap_uv", "drop_last_tile")


def evaluate(gc, plant=None):
	"""(Gbuf, Hbuf) as a call would leave them.  plant None: coordinates subtracted, then scaled (the contract).  Plants: scale_first
	(x * inv_ls - xt * inv_ls); norm_expansion (r^2 = |a|^2 + |b|^2 - 2 <a, b> of the scaled points); m12_unguarded (Matern 1/2 without its
	r > 0 guard: exp(-r) / r at r = 0); inv_ls_by_col (inv_ls[cols[k]], wrapped into range, for inv_ls[k]); no_w1_diag (the Hessian's diagonal
	without psi); no_final_scale (no inv_ls factor after the sum); swap_uv; drop_last_tile (the last m mod 4 test rows never written)."""
	assert plant is None or plant in PLANTS
	T = gc.np_dtype
	W = np.float64 if T == np.float32 else LD
	n, m, d = gc.n, gc.m, gc.d
	x, xt, il = gc.x[:, gc.sel].astype(T), gc.xt[:, gc.sel].astype(T), gc.inv_ls.astype(T)
	if plant == "inv_ls_by_col":
		il = il[[c % d for c in gc.sel]]
	kappa, offset = T(gc.kappa), T(gc.offset)
	u, v = (gc.v, gc.u) if plant == "swap_uv" else (gc.u, gc.v)
	one = np.ones(m, dtype=T)
	c = np.zeros((m, n), dtype=T)
	if gc.alpha is not None:
		c = (one if u is None else u.astype(T))[:, None] * gc.alpha.astype(T)[None, :]
	if gc.Wt is not None:
		c = c + (one if v is None else v.astype(T))[:, None] * gc.Wt[:, :n].astype(T)
	s = np.zeros((m, n), dtype=T)
	e = []
	with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
		for k in range(d):
			if gc.dot:
				e.append((x[None, :, k] * il[k]) + np.zeros((m, 1), dtype=T))
				s = s + (xt[:, k, None] * il[k]) * (x[None, :, k] * il[k])
			else:
				e.append(xt[:, k, None] * il[k] - x[None, :, k] * il[k] if plant == "scale_first" else (xt[:, k, None] - x[None, :, k]) * il[k])
				s = s + e[k] * e[k]
		if plant == "norm_expansion" and not gc.dot:
			xa, xb = x * il, xt * il
			na, nb, acc = np.zeros(n, dtype=T), np.zeros(m, dtype=T), np.zeros((m, n), dtype=T)
			for k in range(d):
				na, nb, acc = na + xa[:, k] * xa[:, k], nb + xb[:, k] * xb[:, k], acc + xb[:, k, None] * xa[None, :, k]
			s = np.maximum(nb[:, None] + na[None, :] - T(2) * acc, T(0))
		chi = np.zeros((m, n), dtype=T)
		if gc.kind == E.SE:
			ex = kappa * np.exp(T(-0.5) * s)
			psi, chi = -ex, ex
		elif gc.kind == E.M12:
			r = np.sqrt(s)
			psi = -kappa * np.exp(-r) / r
			if plant != "m12_unguarded":
				psi = np.where(r > 0, psi, T(0))
		elif gc.kind == E.M32:
			psi = T(-3) * kappa * np.exp(T(np.sqrt(3.0)) * -np.sqrt(s))
		elif gc.kind == E.M52:
			r = np.sqrt(s)
			ex = kappa * np.exp(-(T(np.sqrt(5.0)) * r))
			psi, chi = T(-5.0 / 3.0) * (T(1) + T(np.sqrt(5.0)) * r) * ex, T(25.0 / 3.0) * ex
		elif gc.kind == E.LIN:
			psi = np.full((m, n), kappa, dtype=T)
		else:
			b, p = s + offset, gc.degree
			psi = kappa * T(p) * _ipow(b, p - 1)
			if p >= 2:
				chi = kappa * T(p) * T(p - 1) * _ipow(b, p - 2)
		w1, w2 = c * psi, c * chi
		rows = m - m % GG_TM if plant == "drop_last_tile" else m
		Gbuf = gc.G0.astype(T).copy()
		Hbuf = gc.H0.astype(T).copy() if gc.order == 2 else None
		for k in range(d):
			val = np.sum((w1 * e[k]).astype(W), axis=1).astype(T)
			if plant != "no_final_scale":
				val = val * il[k]
			ck = gc.sel[k]
			Gbuf[:rows, ck] = (Gbuf[:rows, ck] + val[:rows]) if gc.combine == ADD else val[:rows]
			if gc.order == 2:
				for l in range(d):
					term = w2 * e[k] * e[l]
					if k == l and not gc.dot and plant != "no_w1_diag":
						term = term + w1
					val = np.sum(term.astype(W), axis=1).astype(T)
					if plant != "no_final_scale":
						val = val * (il[k] * il[l])
					cl = gc.sel[l]
					Hbuf[:rows, ck, cl] = (Hbuf[:rows, ck, cl] + val[:rows]) if gc.combine == ADD else val[:rows]
	return Gbuf, Hbuf


def _ipow(b, p):
	r = np.ones_like(b)
	for _ in range(p):
		r = r * b
	return r


# ------------------------------------------------------------------------------------------------------------------------------
# the cases
LAYOUT_N, LAYOUT_M, LAYOUT_DIMS = 300, 40, (1, 3, 16)
PLAN_N, PLAN_M, PLAN_D, PLAN_D2 = (1, 255, 256, 257, 513, 1000), (1, 3, 4, 5, 37), (1, 3, 15, 16, 17, 33), (1, 3, 4, 5, 16)
WIDE, WIDE_LDT, WIDE_LDG = 40, 43, 42


def shifts_of(dt):
	return ("offset", "offset_per_column") + (("offset_far",) if dt == "f32" else ())


def _orders(family, d, hess_dims):
	return (1, 2) if family in HESSIAN_FAMILIES and d in hess_dims else (1,)


def layout_cases(dt, family):
	"""The five layouts at n = 300, m = 40 (the training points are `a`, the test points `b` of gram_edge_cases: the duplicates test rows 3 .. 14
	copy training rows, rows 15 .. 20 sit one grid step from one), and the twins of cube and duplicates.  Stationary families; cube and
	duplicates carry the ARD inverse lengthscales, cube_iso (d > 1) ONE inverse lengthscale that is no power of two in every coordinate: the
	kernel scales r^2 once per pair there, another distance loop."""
	out = []
	for d in LAYOUT_DIMS:
		for order in _orders(family, d, LAYOUT_DIMS):
			tag = "%s-%s-d%d-o%d" % (family, dt, d, order)
			for layout in ("cube", "duplicates") + (("cube_iso",) if d > 1 else ()):
				c = D.ard_case(layout.split("_")[0], d, dt, LAYOUT_N, LAYOUT_M)
				if layout == "cube_iso":
					one = (D.ard_inv_ls(1, dt) / np.sqrt(d)).astype(E.DTYPES[dt]).astype(np.float64)
					assert np.frexp(one)[0][0] != 0.5
					c = E.Case(c.layout, d, dt, c.a, c.b, np.repeat(one, d), False)
				base = "%s-%s" % (layout, tag)
				out.append(GradCase(base, family, dt, c.a, c.b, c.inv_ls, order=order))
				for shift in shifts_of(dt):
					tw = D.twin(c, shift)
					out.append(GradCase("%s+%s-%s" % (layout, shift, tag), family, dt, tw.a, tw.b, tw.inv_ls, order=order, twin_of=base, coef_key=base))
			for layout in ("clusters", "tiny_lengthscale", "huge_lengthscale"):
				c = E.make_case(layout, d, dt, LAYOUT_N, LAYOUT_M)
				out.append(GradCase("%s-%s" % (layout, tag), family, dt, c.a, c.b, c.inv_ls, order=order))
	return out


def _cube(d, dt, n, m):
	c = D.ard_case("cube", d, dt, n, m)
	return c.a, c.b, c.inv_ls


def plan_cases(dt, family):
	"""The boundaries of grad_plan and of the kernel's tiles on the cube with ARD lengthscales: every n at m = 5, d = 3; every m at n = 257,
	d = 3; every d at n = 257, m = 5; the corners; the largest shape n = 1000, m = 64.  Order 2 (where the family has it) on its own d list: at
	d = 4, Q = 20, the first output block mixes gradient and Hessian columns and the second holds Hessian columns only."""
	shapes = [(n, 5, 3) for n in PLAN_N] + [(257, m, 3) for m in PLAN_M if m != 5] + [(257, 5, d) for d in PLAN_D if d != 3]
	shapes += [(1, 1, 1), (1000, 37, 33), (1000, 64, 16), (513, 3, 17)]
	out = [GradCase("plan-%s-%s-n%d-m%d-d%d-o1" % (family, dt, n, m, d), family, dt, *_cube(d, dt, n, m)) for (n, m, d) in shapes]
	if family in HESSIAN_FAMILIES:
		shapes2 = [(257, 5, d) for d in PLAN_D2] + [(1000, 37, 4), (513, 1, 16), (1, 3, 5), (256, 4, 3)]
		out += [GradCase("plan-%s-%s-n%d-m%d-d%d-o2" % (family, dt, n, m, d), family, dt, *_cube(d, dt, n, m), order=2) for (n, m, d) in shapes2]
	return out


def form_cases(dt, family):
	"""Every coefficient form (alpha with u, Wt with v, both, each with its scale NULL) at n = 257, m = 5, d = 3; ldw = n + 5 throughout."""
	return [GradCase("form-%s-%s-%s" % (form, family, dt), family, dt, *_cube(3, dt, 257, 5), form=form, order=(2 if family in HESSIAN_FAMILIES else 1))
	        for form in COEF_FORMS if form != "both"]


def column_cases(dt, family):
	"""A column group: d = 5 and d = 16 coordinates as a non-monotone subset of a 40-wide x, the test points stored 43 wide (ldt != ldx), G
	42 wide (ldg > every column), SET onto the sentinel and ADD onto random contents; n = 300, m = 37 (a partial last tile of test rows)."""
	out = []
	for d in (5, 16):
		w, cols, g = D.wide_case("cube", d, dt, 300, 37)
		xt = np.concatenate([w.b, np.full((w.b.shape[0], WIDE_LDT - WIDE), 3.0)], axis=1)
		for order in _orders(family, d, (5,)):
			for combine in (SET, ADD):
				out.append(GradCase("cols-%s-%s-d%d-o%d-%s" % (family, dt, d, order, "add" if combine else "set"), family, dt, w.a, xt, g.inv_ls, cols=cols,
				                    order=order, combine=combine, ldg=WIDE_LDG))
	return out


def exact_cases(dt, family):
	"""n = m = 1 with xt == x, d = 3, the coefficient u alpha alone: G is exactly 0, the off-diagonal of H exactly 0, its diagonal
	c psi(0) inv_ls_k^2 (psi(0) = -kappa for SE, -(5 / 3) kappa for Matern 5/2) to the bound."""
	assert family in STATIONARY_FAMILIES
	x, _, il = _cube(3, dt, 1, 1)
	return [GradCase("exact-%s-%s" % (family, dt), family, dt, x, x.copy(), il, form="alpha_u", order=(2 if family in HESSIAN_FAMILIES else 1))]


def cases(dt, family):
	"""Every case of one family and dtype."""
	out = plan_cases(dt, family) + form_cases(dt, family) + column_cases(dt, family)
	if family in STATIONARY_FAMILIES:
		out = layout_cases(dt, family) + out + exact_cases(dt, family)
	else:
		out += [GradCase("huge_lengthscale-%s-%s-d3" % (family, dt), family, dt, *(lambda c: (c.a, c.b, c.inv_ls))(E.make_case("huge_lengthscale", 3, dt, LAYOUT_N, LAYOUT_M)),
		                 order=2)]
	names = [c.name for c in out]
	assert len(set(names)) == len(names)
	return out


# which planted evaluator each named case must defeat (tests/test_gram_grad_cases_cpu.py asserts every line; "twin": by breaking the
# bit-identity with its centred case, "bound": by exceeding the entrywise bound, "nan": by a NaN in an owned entry, "untouched":
# by leaving owned entries unwritten, which the bound sees as the sentinel)
DEFEATS = {
	"scale_first": [("cube+offset-se-f64-d3-o1", "twin"), ("cube_iso+offset-se-f64-d16-o1", "twin"), ("cube_iso+offset_far-m12-f32-d3-o1", "bound"), ("cube+offset-se-f64-d3-o1", "bound"), ("duplicates+offset-m12-f64-d1-o1", "bound"),
	                ("duplicates+offset-m52-f64-d16-o2", "twin"), ("cube+offset_per_column-m32-f64-d16-o1", "twin"),
	                ("cube+offset-se-f32-d3-o1", "twin"), ("cube+offset_far-se-f32-d3-o1", "bound"), ("duplicates+offset_far-m52-f32-d16-o2", "twin"),
	                ("duplicates+offset_far-m12-f32-d1-o1", "bound")],
	"norm_expansion": [("duplicates+offset-m12-f64-d3-o1", "bound"), ("duplicates+offset-se-f64-d3-o1", "bound"), ("cube+offset_far-m52-f32-d3-o1", "bound"),
	                   ("cube+offset-m32-f64-d16-o1", "twin")],
	"m12_unguarded": [("duplicates-m12-f64-d3-o1", "nan"), ("duplicates-m12-f32-d1-o1", "nan"), ("exact-m12-f64", "nan"), ("exact-m12-f32", "nan")],
	"inv_ls_by_col": [("cols-se-f64-d5-o2-set", "bound"), ("cols-m32-f32-d16-o1-add", "bound"), ("cols-poly3-f64-d5-o2-set", "bound")],
	"no_w1_diag": [("plan-se-f64-n257-m5-d4-o2", "bound"), ("exact-m52-f32", "bound"), ("cols-m52-f64-d5-o2-add", "bound")],
	"no_final_scale": [("plan-se-f64-n257-m5-d3-o1", "bound"), ("plan-lin-f32-n257-m5-d3-o1", "bound"), ("cube-m12-f32-d16-o1", "bound")],
	"swap_uv": [("cube-se-f64-d3-o1", "bound"), ("form-alpha_u-m52-f32", "bound"), ("form-wt_v-poly2-f64", "bound")],
	"drop_last_tile": [("plan-se-f64-n257-m5-d3-o1", "bound"), ("cols-m12-f32-d5-o1-set", "bound"), ("plan-poly7-f64-n1000-m37-d33-o1", "bound")],
}
