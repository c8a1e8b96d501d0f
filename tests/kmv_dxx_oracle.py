"""
NumPy oracle of the matrix-free second-order and standard-deviation input derivatives (stpy_kmv_dxx; IterativeGaussianProcess.mean_std_grad /
mean_value_grad_hessian / mean_gradient_hessian / ucb_optimize): the dense statement of stpy_kmv_dxx in longdouble with per-entry error bounds
and a working-precision emulation, and the dense float64 posterior derivatives with the bounds a CG solve of true relative residual 2 tol
leaves on them (an extension of kmv_oracle.posterior_bounds).  Shared by the CPU and the GPU tests; nothing here touches the GPU or the library.

stpy_kmv_dxx, per query point i and coefficient row c, with e_k = (a_i - b_j)[cols[k]] inv_ls[k], rho = sum e_k^2, chi = 2 dphi/drho, psi = 2 dchi/drho:
  gradient block   out[c, i, k]                    = il_k sum_j V_cj kappa chi e_k                                    k < d
  value            out[c, i, d]                    =      sum_j V_cj kappa phi
  Hessian block    out[c, i, d + 1 + k(k+1)/2 + l] = il_k il_l sum_j V_cj kappa (psi e_k e_l + chi [k == l])          l <= k < d
Bounds: the first two blocks carry the bounds of stpy_kmv_dx (pathwise_oracle.kmv_dx_bound).  The Hessian block is bounded on the SUM OF
MAGNITUDES of its two parts, because they cancel on the diagonal:
  2 eps (q + d + 12) SH,   SH = sum_j |V_cj| kappa il_k il_l (|psi e_k e_l| + |chi| [k == l])
(d + 8) from the evaluator's contract on a kernel value, four further roundings (two products, the sum, the scale), q for the summation.
"""
import numpy as np
import scipy.linalg as sla

from tests import kmv_oracle as KO
from tests import nystrom_oracle as NO
from tests import pathwise_oracle as PO
from tests import slq_oracle as SO

HESSIAN_KINDS = ("se", "matern52")


def ncol(d):
	return 1 + d + d * (d + 1) // 2


def tri_index(d):
	"""(k, l) of the Hessian block's columns, in order: row by row of the lower triangle."""
	return [(k, l) for k in range(d) for l in range(k + 1)]


def _psi(kind, rho):
	"""psi = 2 dchi/drho in rho's dtype (SE and Matern 5/2: finite at rho == 0)."""
	dt = rho.dtype.type
	if kind == "se":
		return np.exp(dt(-0.5) * rho)
	if kind == "matern52":
		return dt(25.0) / dt(3.0) * np.exp(-np.sqrt(rho) * dt(SO.SQRT5))
	raise ValueError("no second derivative for kind %r (singular at r = 0)" % (kind,))


def kmv_dxx_dense(kind, a, b, inv_ls, V, cols=None, kappa=1.0, dtype=np.longdouble, block=64):
	"""stpy_kmv_dxx stated densely in ``dtype`` (subtract first, then scale): (out (t, n, ncol(d)), S0, S1, SK, SH).  S0 (t, n, d), S1 (t, n, d),
	SK (t, n) are those of pathwise_oracle.kmv_dx_dense; SH (t, n, d (d + 1) / 2) is the sum of magnitudes of the Hessian block (float64)."""
	if kind not in HESSIAN_KINDS:
		raise ValueError("no second derivative for kind %r (singular at r = 0)" % (kind,))
	first, S0, S1, SK = PO.kmv_dx_dense(kind, a, b, inv_ls, V, cols=cols, kappa=kappa, dtype=dtype)
	a = np.asarray(a, dtype=dtype)
	b = np.asarray(b, dtype=dtype)
	if cols is not None:
		a, b = a[:, list(cols)], b[:, list(cols)]
	il = np.asarray(inv_ls, dtype=dtype)
	V = np.asarray(V, dtype=dtype)
	t, q = V.shape
	n, d = a.shape
	kap = dtype(kappa)
	out = np.zeros((t, n, ncol(d)), dtype=dtype)
	out[:, :, :d + 1] = first
	SH = np.zeros((t, n, d * (d + 1) // 2))
	aV = np.abs(V).astype(np.float64)
	il64 = il.astype(np.float64)
	for i0 in range(0, n, block):
		sl = slice(i0, i0 + block)
		e = (a[sl, None, :] - b[None, :, :]) * il                                      # (bl, q, d)
		rho = np.zeros(e.shape[:2], dtype=dtype)
		for k in range(d):
			rho = e[:, :, k] * e[:, :, k] + rho
		wchi = kap * SO._chi(kind, rho) if q else np.zeros(rho.shape, dtype=dtype)
		wpsi = kap * _psi(kind, rho) if q else np.zeros(rho.shape, dtype=dtype)
		for p, (k, l) in enumerate(tri_index(d)):
			Bk = wpsi * e[:, :, k] * e[:, :, l]
			mag = np.abs(Bk).astype(np.float64)
			if k == l:
				Bk = Bk + wchi
				mag = mag + np.abs(wchi).astype(np.float64)
			out[:, sl, d + 1 + p] = (il[k] * il[l]) * (V @ Bk.T)
			SH[:, sl, p] = il64[k] * il64[l] * (aV @ mag.T)
	return out, S0, S1, SK, SH


def kmv_dxx_bound(q, d, eps, S0, S1, SK, SH):
	"""(t, n, ncol(d)) bound on |device - truth|: the stpy_kmv_dx bound on the first d + 1 columns, 2 eps (q + d + 12) SH on the Hessian block."""
	t, n = SK.shape
	bnd = np.zeros((t, n, ncol(d)))
	bnd[:, :, :d + 1] = PO.kmv_dx_bound(q, d, eps, S0, S1, SK)
	bnd[:, :, d + 1:] = 2 * eps * (q + d + 12) * SH
	return bnd


def kmv_dxx_emulated(kind, a, b, inv_ls, V, dtype, cols=None, kappa=1.0):
	"""The subtract-first evaluation with every operation rounded to the working ``dtype`` (what the device does, up to summation order)."""
	return kmv_dxx_dense(kind, np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype), np.asarray(inv_ls, dtype=dtype), np.asarray(V, dtype=dtype),
						 cols=cols, kappa=kappa, dtype=dtype)[0]


def full_hessian(tri, d):
	"""(..., d (d + 1) / 2) lower triangles -> (..., d, d) symmetric matrices."""
	H = np.zeros(tri.shape[:-1] + (d, d), dtype=tri.dtype)
	for p, (k, l) in enumerate(tri_index(d)):
		H[..., k, l] = tri[..., p]
		H[..., l, k] = tri[..., p]
	return H


# ------------------------------------------------------------------------------------------------------------ posterior derivatives
def kernel_dxx(kind, xt, x, gamma, kappa=1.0, cols=None):
	"""d2 k(xt_i, x_j) / d xt_i d xt_i as (M, n, width, width) in float64 (zero on the columns the kernel does not read)."""
	xt, x = np.asarray(xt, dtype=np.float64), np.asarray(x, dtype=np.float64)
	width = xt.shape[1]
	sel = list(cols) if cols is not None else list(range(width))
	il = np.ones(len(sel)) / np.asarray(gamma, dtype=np.float64)
	e = (xt[:, None, sel] - x[None, :, sel]) * il
	rho = np.sum(e * e, axis=2)
	core = kappa * _psi(kind, rho)[:, :, None, None] * e[:, :, :, None] * e[:, :, None, :]
	core = core + kappa * SO._chi(kind, rho)[:, :, None, None] * np.eye(len(sel))[None, None]
	out = np.zeros((xt.shape[0], x.shape[0], width, width))
	out[np.ix_(range(xt.shape[0]), range(x.shape[0]), sel, sel)] = core * il[None, None, :, None] * il[None, None, None, :]
	return out


# safety on the first-order propagation through 1 / (2 std): with var >= 100 b_var the neglected second-order terms are below 2 % of the first-order ones
SECOND_ORDER = 1.02
VAR_MARGIN = 100.0


def posterior_deriv_bounds(kind, x, y, xt, gamma, s, tol, eps, cols=None, kappa=1.0, hessian=True):
	"""The dense float64 posterior, its input derivatives and per-entry bounds for a CG route whose solves have TRUE relative residual <= 2 tol in
	arithmetic of unit roundoff eps.  Returns a dict:
	  mu, var (M,), b_mu, b_var (M,)                  kmv_oracle.posterior_bounds
	  dmu (M, width), b_dmu                            d mu / dx:   |A^-1 h_ik| 2 tol |y| (h_ik = d_k k*_i, the kernel-derivative vector) + the gradient
	                                                   bound of stpy_kmv_dx on (x*, X, alpha)
	  H (M, width, width), b_H  (``hessian``)          the same with h_ikl = d_k d_l k*_i and the Hessian bound of stpy_kmv_dxx
	  dstd (M, width), b_dstd, dvar, b_dvar            var = kappa - k*^T w, d_k var = -2 T_k, T_k = sum_j w_j d_k k_j; the device's w~ = w + A^-1 e, |e| <= 2 tol |k*|:
	                                                   |T~_k - T_k| <= |A^-1 g_k| 2 tol |k*| (g_k = h_ik) + the gradient bound of the paired-weight
	                                                   sum on (x*, X, w_i) (the same arithmetic as stpy_kmv_dx: difference, scale, chi, product, sum);
	                                                   d std = d var / (2 std), to first order
	                                                   |d std~ - d std| <= b_dvar / (2 std) + |d std| b_var / (2 var), times SECOND_ORDER.
	The propagation needs var >= VAR_MARGIN b_var: ``ok`` (M,) says where that holds; it is a condition on the test POINTS (see test_points)."""
	x, xt = np.asarray(x, dtype=np.float64), np.asarray(xt, dtype=np.float64)
	mu, var, b_mu, b_var = KO.posterior_bounds(kind, x, y, xt, gamma, s, tol, eps, cols, kappa)
	mu, var, b_mu, b_var = mu[:, 0], var[:, 0], b_mu[:, 0], b_var[:, 0]
	n, width = x.shape
	M = xt.shape[0]
	sel = list(cols) if cols is not None else list(range(width))
	d = len(sel)
	il = np.ones(d) / np.asarray(gamma, dtype=np.float64)
	A = NO.kernel(kind, x, x, gamma, kappa, cols) + s * s * np.eye(n)
	Ks = NO.kernel(kind, x, xt, gamma, kappa, cols)                                       # (n, M)
	c = sla.cho_factor(A, lower=True)
	alpha = sla.cho_solve(c, np.asarray(y, dtype=np.float64).reshape(-1, 1))[:, 0]
	W = sla.cho_solve(c, Ks)                                                              # (n, M)
	dK = PO.kernel_dx(kind, xt, x, gamma, kappa, cols)                                    # (M, n, width)
	ynorm, knorm = np.linalg.norm(y), np.linalg.norm(Ks, axis=0)
	dB = sla.cho_solve(c, dK.transpose(1, 0, 2).reshape(n, -1)).reshape(n, M, width)      # A^-1 h_ik
	dBn = np.linalg.norm(dB, axis=0)                                                      # (M, width)
	out = dict(mu=mu, var=var, b_mu=b_mu, b_var=b_var, ok=var >= VAR_MARGIN * b_var)
	# the mean's gradient
	_, S0, S1, SK = PO.kmv_dx_dense(kind, xt, x, il, alpha.reshape(1, -1), cols=cols, kappa=kappa, dtype=np.float64)
	kb = PO.kmv_dx_bound(n, d, eps, S0, S1, SK)[0]                                        # (M, d + 1)
	out["dmu"] = np.einsum("ink,n->ik", dK, alpha)
	b = dBn * 2 * tol * ynorm
	b[:, sel] += kb[:, :d]
	out["b_dmu"] = b
	# the standard deviation's gradient
	T = np.einsum("ink,ni->ik", dK, W)
	bT = dBn * 2 * tol * knorm[:, None]
	for i in range(M):
		_, S0, S1, SK = PO.kmv_dx_dense(kind, xt[i:i + 1], x, il, W[:, i].reshape(1, -1), cols=cols, kappa=kappa, dtype=np.float64)
		bT[i, sel] += PO.kmv_dx_bound(n, d, eps, S0, S1, SK)[0, 0, :d]
	std = np.sqrt(np.maximum(var, 0.0))
	out["dvar"], out["b_dvar"] = -2.0 * T, 2.0 * bT
	with np.errstate(divide="ignore", invalid="ignore"):
		out["dstd"] = np.where(std[:, None] > 0, out["dvar"] / (2.0 * std[:, None]), 0.0)
		out["b_dstd"] = SECOND_ORDER * (out["b_dvar"] / (2.0 * std[:, None]) + np.abs(out["dstd"]) * (b_var / (2.0 * var))[:, None])
	if hessian and kind in HESSIAN_KINDS:
		ddK = kernel_dxx(kind, xt, x, gamma, kappa, cols)                                 # (M, n, width, width)
		out["H"] = np.einsum("inkl,n->ikl", ddK, alpha)
		ddB = sla.cho_solve(c, ddK.transpose(1, 0, 2, 3).reshape(n, -1)).reshape(n, M, width, width)
		bH = np.linalg.norm(ddB, axis=0) * 2 * tol * ynorm
		SH = kmv_dxx_dense(kind, xt, x, il, alpha.reshape(1, -1), cols=cols, kappa=kappa, dtype=np.float64)[4][0]          # (M, d (d + 1) / 2)
		bH[np.ix_(range(M), sel, sel)] += full_hessian(2 * eps * (n + d + 12) * SH, d)
		out["b_H"] = bH
	return out


def test_points(idx, dtype=np.float64, m_test=37):
	"""(x, y, xt) of a case of kmv_oracle.PCG_CASES with the test points of the derivative tests: the case's own data, and test points uniform in
	the data's box [-1, 1]^width with ONE coordinate that the kernel reads pushed outside it, to +-(1 + gamma u), u uniform in [0.75, 1.75]: three quarters to
	one and three quarter lengthscales off a face of the box, where the posterior still depends on the data (k* is not small) and the variance is far
	above the solver's error on it -- the propagation through 1 / (2 std) needs var >= VAR_MARGIN b_var (tests/test_kmv_dxx_cpu.py checks that it
	holds at every point, for both settings)."""
	kind, n, d, gamma, r, cols = KO.PCG_CASES[idx]
	x, y, _ = KO.case_data(idx, dtype)
	rng = np.random.RandomState(8800 + idx)
	xt = rng.uniform(-1, 1, size=(m_test, x.shape[1]))
	sel = list(cols) if cols else list(range(x.shape[1]))
	which = rng.randint(0, len(sel), size=m_test)
	side = rng.randint(0, 2, size=m_test) * 2 - 1
	off = rng.uniform(0.75, 1.75, size=m_test)
	for i in range(m_test):
		xt[i, sel[which[i]]] = side[i] * (1.0 + gamma * off[i])
	if np.dtype(dtype) == np.float32:
		xt = xt.astype(np.float32).astype(np.float64)
	return x, y, xt
