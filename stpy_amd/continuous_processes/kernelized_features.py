"""
Drop-in for ``stpy.continuous_processes.kernelized_features.KernelizedFeatures``
(reference: kernelized_features.py:12-54 ctor, :56-106 beta / embed / kernel /
logdet_ratio / effective_dim, :108-138 add_data_point / fit_gp, :164-246 get_invV / precompute, :248-298 theta_mean /
mean_std / ucb / lcb, :300-336 sample_matheron / sample_theta, :537-562 sample / sample_and_max / get_kernel / residuals).

As in the reference the class derives from ``GaussianProcess`` and does not run the base constructor: ``log_marginal(kernel, X,
weight)`` (the evidence of ``kernel`` on the stored data, with its analytic gradient), ``optimize_params`` (needs a
``kernel_object`` attribute, which the reference never sets either), ``load_data`` ... are the inherited device paths.

Ridge regression on a finite feature map Phi (n x m), e.g. random Fourier features:

  primal (default, or n >= m):  V = Phi^T Phi + s^2 lam I,  theta = V^-1 Phi^T y,  std = s sqrt(diag(Phi* V^-1 Phi*^T))
  dual (primal=False, n < m):   K = Phi Phi^T + s^2 lam I,  theta = Phi^T K^-1 y,  std^2 = (|phi*|^2 - phi*^T Phi^T K^-1 Phi phi*) / lam
                                -- the GP path on the linear kernel of the features (kernelized_features.py:229-235, :252-254, :285)

Device mapping -- every contraction is the NT MFMA GEMM because the embedding is produced TRANSPOSED (Phi^T, m x n:
``embed_t``), and in the primal form Phi is STREAMED: row slabs of x are embedded one at a time (``slab_bytes`` of features live,
2 GB by default) and accumulated, so the n x m feature matrix is never materialised (at BASELINE config 5's shape it is 34 GB).
That requires an embedding that acts ROW BY ROW (each output row depends on its own input row only); every embedding of
``stpy_amd.embeddings`` does, and a fit of more than one slab checks it on the first row.
    V          += Phi_slab^T Phi_slab   stpy_syrk(mode "+="), lower tiles; + s^2 lam on the diagonal: stpy_combine
    Phi^T y    += Phi_slab^T y_slab     stpy_predict (row sums against y_slab) + stpy_combine(ADD)
    V = L L^T                           stpy_potrf  (the reference takes pinverse(V); V is SPD for s, lam > 0)
    theta                               stpy_trsv forward + backward
    X = Phi* L^-T, mean = X u, std      stpy_trsm_right_lt, stpy_predict, stpy_predict_finish
    samplers                            stpy_potri -> stpy_potrf -> stpy_tril (once per factor) -> stpy_gemm_nt (chol(V^-1) s r, the reference's
                                        own factor of the covariance, so a seeded run draws the same theta); Matheron: stpy_gram + stpy_potrf +
                                        stpy_trsm_right_lt + stpy_gemm_nt
Standard-normal draws are taken exactly as the reference takes them (torch.normal on the CPU generator, shape (basis, size)).

``add_data_point`` queues points as the reference does (:108-113) and the next prediction folds them in: k new rows cost their
embedding, one k-deep ``+=`` product and one m x m refactorisation (the reference's rank-one Woodbury / Schur updates of the
explicit inverse, :181-221, call ``add_points`` with the wrong arity and raise).  ``add_data_point(x, y, iterative=True)`` replaces
the refactorisation by a rank-k update of the resident factor (``stpy_chol_update``, csrc/cholupdate.hip: V' = V + W W^T with
W = Phi_new^T, one pass over L, O(m^2 k)) whenever every queued point asked for it, the primal form is active, a factor of the same
dtype and the same s^2 lam is resident and the batch has at most ``update_max_rank`` rows; V_acc and Phi^T y are kept exact as on
the refit path, theta is two ``stpy_trsv`` on the updated factor, and a failed update (status word, hand-off error) falls back to
the refit of V_acc.  The sampler's factor chol(V^-1) is kept on the resident factor; a one-row update downdates it
(V'^-1 = V^-1 - u u^T, u = V^-1 w / sqrt(1 + w^T V^-1 w): two ``stpy_trsv`` and ``stpy_chol_update`` with sign -1), a wider one
drops it.  The cvxpy / MOSEK constrained fits (:338-435) are outside the hot path.

Input gradients (csrc/rffgrad.hip).  Both forms have mu = phi^T theta and sigma^2 = phi^T Z phi with a symmetric Z (primal
s^2 V^-1, dual (I - Phi^T K^-1 Phi) / lam), so for upstream gradients g_mu, g_sigma
    grad_x [g_mu mu + g_sigma sigma](x_t) = sum_j C_tj d phi_tj / dx,     C_t = g_mu_t theta + (g_sigma_t / sigma_t) (Phi_t Z)
which is ONE ``stpy_rff_grad`` launch on the embedding's operands: ``mean_std`` / ``mean_var`` / ``mean`` / ``ucb`` / ``lcb``
differentiate through a test tensor with requires_grad, and ``sample_and_optimize`` (:501-535) climbs a sampled
f = phi^T theta from all starts at once (the shared coefficient row, values and gradients from the same launch).  Phi_t Z is
one product with V^-1 (K^-1 in the dual form) from ``stpy_potri``, kept per fit: the factor's order is not a multiple of 128
in general, which the right solve ``stpy_trsm_right_ln`` needs.  ``mean_std_grad``, ``mean_gradient_hessian``,
``gradient_mean_var`` and ``ucb_optimize`` still raise (see ``_no_input_gradients``).

Reference quirks kept (pinned by goldens G12 / G15): ``kernel`` and ``get_kernel`` use a linear kernel object built with the
default d = 1, so only the FIRST feature enters (:51, :93-97, :553-557); ``logdet_ratio`` in the primal form reads the
placeholder ``K = ones(1, 1)`` (:25, :99-101); ``get_invV`` in the dual form builds V from that same first-column kernel of
Q^T (:167-172), which is what ``sample_theta`` then draws from.
"""
import math

import numpy as np
import torch

from .. import _lib
from ..kernels import KernelFunction
from .gauss_procc import GaussianProcess, ResidentFactor, _PosteriorFn, _draw_starts, _multistart_maximize, _wants_grad


class KernelizedFeatures(GaussianProcess):

	def __init__(self, embedding, m, s=0.001, lam=1., d=1, diameter=1.0, theta_norm=1.0, verbose=True, groups=None,
				 bounds=None, scale=1.0, kappa=1.0, poly=2, primal=True, beta_fun=None, bound=1):
		self.s = s
		self.lam = lam
		self.primal = primal
		self.x = None
		self.y = None
		self.mu = 0.0
		self.m = torch.from_numpy(np.array(m))
		self.fitted = False
		self.data = False
		self.d = d
		self.n = 0
		self.bounds = bounds
		self.groups = groups
		self.diameter = diameter
		self.theta_norm = theta_norm
		self.verbose = verbose
		self.admits_first_order = True
		self.embedding = embedding
		self.embedding_map = embedding
		self.kappa = kappa
		self.scale = scale
		self.poly = poly
		self.to_add = []
		self.prior_mean = 0
		self.dual = False
		self.beta_fun = beta_fun
		self.bound = bound
		# what the inherited GaussianProcess methods read (the reference leaves these unset and its inherited log_marginal
		# stops at ``self.loss``)
		self.loss = 'squared'
		self.back_prop = True
		self.max_size = 10000
		self.clamp_variance = False
		self.kernel_object = None
		self.nb = 0
		self.slab_bytes = 2 << 30          # features held at a time while V and Phi^T y are accumulated (fit_gp)
		self.update_max_rank = 128         # widest batch of add_data_point(iterative=True) that updates the factor instead of refitting
		self._xd = self._yd = None
		self._Sigma = None
		self._factor = self._theta = None                         # ResidentFactor of V (primal, m x m) or K (dual, n x n); z = L^-1 rhs
		self._Vacc = self._rhs = self._part = None                # accumulated Phi^T Phi (lower tiles) and Phi^T y
		self._ridge = None                                        # s^2 lam the resident primal factor was built with
		self._PhiT = None                                         # dual form: Phi^T (m, n), kept (n < m)

	# ------------------------------------------------------------------ small API mirrors
	def description(self):
		return "Custom Features object"

	def embed(self, x):
		return self.embedding.embed(x)

	def set_embedding(self, embed):
		self.embedding_map = embed

	def get_basis_size(self):
		return int(torch.sum(self.m))

	def set_basis_size(self, m):
		self.m = m

	@property
	def K(self):
		"""kernelized_features.py:25 (primal: the placeholder ones(1, 1)) / :232 (dual: Phi Phi^T + s^2 lam I)."""
		if not (self.dual and self.fitted):
			return torch.ones(size=(1, 1)).double()
		return _lib.like_input(self._dual_K(), self.x)

	def _embed_t(self, xd):
		"""Phi^T on the device, (m, n)."""
		if hasattr(self.embedding, "embed_t"):
			return self.embedding.embed_t(xd)
		return _lib.to_device(self.embedding.embed(xd)).T.contiguous()       # generic embeddings: one transpose copy

	def _first_feature_kernel(self, x, y, diag_add=0.0):
		"""(|y|, |x|) linear kernel of the FIRST feature only (see the module header), + diag_add on the diagonal; device tensor."""
		ex = _lib.to_device(self.embed(_lib.to_device(x)))[:, :1].contiguous()
		ey = _lib.to_device(self.embed(_lib.to_device(y)), ex.dtype)[:, :1].contiguous()
		out = torch.empty((ey.shape[0], ex.shape[0]), dtype=ex.dtype, device=ex.device)
		_lib.gemm_nt(ey, ex, out)
		if diag_add != 0.0:
			_lib.combine(out, out, _lib.OUT_SET, diag_add)
		return out

	def kernel(self, x, y):
		"""kernelized_features.py:93-97."""
		return _lib.like_input(self._first_feature_kernel(x, y), x)

	def get_kernel(self):
		"""kernelized_features.py:553-557."""
		return _lib.like_input(self._first_feature_kernel(self.x, self.x, float(self.s) ** 2 * float(self.lam)), self.x)

	def logdet_ratio(self):
		"""kernelized_features.py:99-101: logdet(self.K) - logdet(s^2 lam I_m)."""
		self.precompute()
		m = self.get_basis_size()
		ld = 2.0 * float(_lib.logdet_quad(self._L)[0].item()) if (self.dual and self.fitted) else 0.0        # primal: K is the ones(1, 1) placeholder
		return torch.tensor(ld - m * math.log(float(self.s) ** 2 * float(self.lam)), dtype=torch.float64)

	def effective_dim(self, xtest):
		"""kernelized_features.py:103-106: tr((Phi^T Phi + lam I)^-1 Phi^T Phi) = m - lam tr((Phi^T Phi + lam I)^-1)
		(the reference line calls torch.solve, which current torch no longer has; this is what it computes)."""
		xt = _lib.to_device(xtest)
		PhiT = _lib.to_device(self._embed_t(xt), xt.dtype)
		if PhiT.stride(1) != 1:
			PhiT = PhiT.contiguous()
		m = PhiT.shape[0]
		A = torch.empty((m, m), dtype=PhiT.dtype, device=PhiT.device)
		_lib.gemm_nt(PhiT, PhiT, A, lower_only=True)
		_lib.combine(A, A, _lib.OUT_SET, float(self.lam))
		L, winv = self._chol(A, "effective_dim: Phi^T Phi + lam I")
		inv = _lib.potri(L, winv)
		return torch.tensor(m - float(self.lam) * float(_lib.trace_dot(inv)[0].item()), dtype=torch.float64)

	def beta(self, delta=0.1, norm=None):
		"""kernelized_features.py:56-76."""
		if norm is None:
			norm = self.theta_norm
		if self.beta_fun is None:
			return 2.0
		if self.beta_fun == "theory":
			# bound lam + logdet(Q^T Q / s^2 + lam I) - logdet(lam I) + 2 log(1/delta), from the resident factor:
			# logdet(Q^T Q + c I_m) = logdet(V) in the primal form, logdet(K) + (m - n) log c in the dual one (c = s^2 lam)
			self.precompute()
			m = self.get_basis_size()
			c = float(self.s) ** 2 * float(self.lam)
			ldV = 2.0 * float(_lib.logdet_quad(self._L)[0].item()) + ((m - self.n) * math.log(c) if self.dual else 0.0)
			val = float(self.bound) * float(self.lam) + ldV - m * math.log(float(self.s) ** 2) - m * math.log(float(self.lam)) + 2 * np.log(1 / delta)
			return torch.tensor(val, dtype=torch.float64)
		return self.beta_fun(self.K, delta=delta, norm=norm)

	# ------------------------------------------------------------------ fit
	def add_data_point(self, x, y, iterative=False):
		"""kernelized_features.py:108-113: the first point fits, later ones are queued and folded in by the next ``precompute``.
		``iterative=True`` asks that fold for a rank-k update of the resident factor instead of a refactorisation (see the module
		header for when it is taken); entries queued without it keep the reference's [x, y] form."""
		if self.n == 0:
			self.fit_gp(x, y)
		else:
			self.to_add.append([x, y, True] if iterative else [x, y])
			self.fitted = False

	add_data = add_data_point

	def add_points(self, d):
		"""kernelized_features.py:140-147."""
		x, y = d
		if self.x is not None:
			self.x = torch.cat((self.x, x), dim=0)
			self.y = torch.cat((self.y, y), dim=0)
		else:
			self.x = x
			self.y = y

	def fit(self, x=None, y=None):
		self.fit_gp(self.x if x is None else x, self.y if y is None else y)

	def fit_gp(self, x, y):
		"""kernelized_features.py:118-138."""
		self.x, self.y = x, y
		self.n = list(x.size())[0]
		self.d = list(x.size())[1]
		self.dual = (self.n < self.get_basis_size()) and not self.primal
		self.data = True
		self.fitted = False
		self.to_add = []
		self._Vacc = self._rhs = self._part = self._PhiT = None
		self._factor = self._theta = None
		self.precompute()
		return None

	def precompute(self):
		"""kernelized_features.py:176-246."""
		if self.fitted or not self.data:
			return
		if len(self.to_add) > 0 and self._Vacc is not None and not self.dual:
			# primal: the accumulated normal equations are extended by the queued rows
			iterative = all(len(p) > 2 and p[2] for p in self.to_add)
			newx = torch.cat([p[0] for p in self.to_add], dim=0)
			newy = torch.cat([p[1] for p in self.to_add], dim=0)
			self.to_add = []
			self.add_points((newx, newy))
			self.n = list(self.x.size())[0]
			self._xd = self._yd = None
			dtype = self._Vacc.dtype
			xn, yn = _lib.to_device(newx, dtype), _lib.to_device(newy, dtype).reshape(-1)
			F = self._factor
			if (iterative and F is not None and F.L.dtype == dtype and self._ridge == float(self.s) ** 2 * float(self.lam)
					and 0 < xn.shape[0] <= int(self.update_max_rank)):
				if self._update_factor(xn, yn):
					return
			else:
				self._accumulate(xn, yn, first=False)
			self._solve_normal_equations()
			return
		if len(self.to_add) > 0:
			for p in self.to_add:
				self.add_points((p[0], p[1]))
			self.to_add = []
			self.n = list(self.x.size())[0]
			self.dual = (self.n < self.get_basis_size()) and not self.primal          # (check_conversion, :149-162)
		xd = _lib.to_device(self.x)
		yd = _lib.to_device(self.y, xd.dtype).reshape(-1)
		self._xd, self._yd = xd, yd.reshape(-1, 1)
		if self.dual:
			self._fit_dual(xd, yd)
		else:
			self._Vacc = self._rhs = self._part = None
			self._accumulate(xd, yd, first=True)
			self._solve_normal_equations()

	def _accumulate(self, xd, yd, first):
		"""V_acc (+)= Phi^T Phi (lower tiles) and rhs (+)= Phi^T y over row slabs of xd; ``first``: the buffers are (re)created."""
		n = xd.shape[0]
		esz = xd.element_size()
		m = None if first else self._Vacc.shape[0]
		rows = n if first else max(128, (int(self.slab_bytes) // (m * esz)) // 128 * 128)
		r0 = 0
		while r0 < n:
			take = min(4096 if m is None else rows, n - r0)          # (first slab of a fit: a probe that tells the feature count)
			PhiT = _lib.to_device(self._embed_t(xd[r0:r0 + take]), xd.dtype)            # (m, take)
			if PhiT.stride(1) != 1:
				PhiT = PhiT.contiguous()
			if m is None:
				m = PhiT.shape[0]
				rows = max(128, (int(self.slab_bytes) // (m * esz)) // 128 * 128)
				self._Vacc = torch.empty((m, m), dtype=xd.dtype, device=xd.device)
				self._rhs = torch.empty((1, m), dtype=xd.dtype, device=xd.device)
				self._part = torch.empty((1, m), dtype=xd.dtype, device=xd.device)
				if take < n:
					# slab-wise embedding is only the embedding of the whole set if the map acts row by row: row 0 alone
					# must reproduce column 0 of the slab
					alone = _lib.to_device(self._embed_t(xd[0:1]), xd.dtype).reshape(-1)
					if not torch.allclose(alone, PhiT[:, 0], rtol=1e-6 if xd.dtype == torch.float32 else 1e-12, atol=1e-6 if xd.dtype == torch.float32 else 1e-12):
						raise ValueError("KernelizedFeatures: the embedding does not act row by row (embed(x[0:1]) differs from the first row of "
										 "embed(x[0:%d])); the streaming fit needs that -- raise slab_bytes so that one slab holds all rows" % take)
			V = self._Vacc
			# V (+)= Phi_slab^T Phi_slab, lower tiles only: mode 0 for the first slab of a fit, 2 (accumulate) afterwards
			# (fp32 slabs of 2048 features and more: the slab is split once into bf16 planes in a workspace and every output tile reads those)
			_lib.syrk(PhiT, V, 0 if first else 2)
			# Phi_slab^T y_slab: row sums of Phi^T against y
			ys = yd[r0:r0 + take]
			tgt = self._rhs if first else self._part
			_lib.predict(PhiT, ys, tgt)
			if not first:
				_lib.combine(self._rhs, self._part, _lib.OUT_ADD)
			first = False
			r0 += take
			del PhiT

	def _update_factor(self, xn, yn):
		"""The k rows (xn, yn) folded into the resident primal factor by a rank-k update: V_acc += W W^T and rhs += W yn exactly as the
		refit path does (W = Phi_new^T, (m, k), embedded once), L <- chol(L L^T + W W^T) in place (stpy_chol_update), z and theta from
		two vector solves, the derived inverse / reversed factor dropped.  A resident sampler factor C = chol(V^-1) follows a one-row
		update by the downdate V'^-1 = V^-1 - u u^T, u = L^-T p / sqrt(1 + p^T p), p = L^-1 w (the OLD factor); a wider update drops it,
		as does a downdate whose status word is not 0.  Returns False -- V_acc and rhs are up to date, the factor is not -- when the
		update reports a failing pivot or a hand-off error: the caller refits."""
		F = self._factor
		W = _lib.to_device(self._embed_t(xn), xn.dtype)                   # (m, k)
		if W.stride(1) != 1:
			W = W.contiguous()
		_lib.syrk(W, self._Vacc, 2)
		_lib.predict(W, yn, self._part)
		_lib.combine(self._rhs, self._part, _lib.OUT_ADD)
		U = None
		if F._sampler is not None and W.shape[1] == 1:
			p = _lib.trsv(F.L, F.winv, W)
			q = _lib.trsv(F.L, F.winv, p, trans=1)
			U = (q * torch.rsqrt(1.0 + _lib.trace_dot(u=p, v=p)[1])).reshape(-1, 1)          # (one scalar, on the device)
		info = _lib.chol_update(F.L, F.winv, W, 1)                        # (W is scratch from here on)
		info_c = None if U is None else _lib.chol_update(F._sampler[0], F._sampler[1], U, -1)
		F._alpha = F._inverse = F._reversed = None
		self.fitted = False
		theta = F.solve(self._rhs)
		ok = int(info.item()) == 0
		try:
			_lib.check_async("KernelizedFeatures: stpy_trsv")       # a hand-off wait that gave up has poisoned u / theta with NaN
		except _lib.StpyHipError:
			ok = False
		if not ok:
			return False
		if info_c is None or int(info_c.item()) != 0:
			F._sampler = None                                             # the next draw factors V^-1 afresh
		self._theta = theta
		self.fitted = True
		return True

	def _chol(self, A, what):
		"""In-place stpy_potrf of A; returns (A, winv).  Raises LinAlgError (and leaves the object unfitted) on a failing pivot."""
		winv, info = _lib.potrf(A, self.nb)
		self._check_info(info, "KernelizedFeatures: " + what + " is not positive definite (leading minor %d)")
		return A, winv

	def _solve_normal_equations(self):
		"""V = V_acc + s^2 lam I -> Cholesky, u = L^-1 (Phi^T y), theta = L^-T u."""
		V = torch.empty_like(self._Vacc)
		# V = V_acc, then + s^2 lam on the diagonal (one pass of the elementwise kernel)
		_lib.combine(V, self._Vacc, _lib.OUT_SET, float(self.s) ** 2 * float(self.lam))
		self.fitted = False
		F = ResidentFactor(*self._chol(V, "Phi^T Phi + s^2 lam I"))
		theta = F.solve(self._rhs)
		_lib.check_async("KernelizedFeatures: stpy_trsv")           # a hand-off wait that gave up has poisoned u / theta with NaN
		self._factor, self._theta = F, theta
		self._ridge = float(self.s) ** 2 * float(self.lam)
		self.fitted = True

	def _dual_K(self):
		"""Phi Phi^T + s^2 lam I (n x n, full) from the kept Phi^T."""
		Phi = self._PhiT.t().contiguous()                                 # (n, m); n < m
		n = Phi.shape[0]
		K = torch.empty((n, n), dtype=Phi.dtype, device=Phi.device)
		_lib.gemm_nt(Phi, Phi, K)
		_lib.combine(K, K, _lib.OUT_SET, float(self.s) ** 2 * float(self.lam))
		return K

	def _fit_dual(self, xd, yd):
		"""kernelized_features.py:229-235, :252-254: K = Q Q^T + s^2 lam I -> Cholesky, z = L^-1 y, theta = Q^T K^-1 y."""
		PhiT = _lib.to_device(self._embed_t(xd), xd.dtype)                # (m, n)
		if PhiT.stride(1) != 1:
			PhiT = PhiT.contiguous()
		self._PhiT = PhiT
		self.fitted = False
		F = ResidentFactor(*self._chol(self._dual_K(), "Phi Phi^T + s^2 lam I"))
		alpha = F.solve(yd)
		_lib.check_async("KernelizedFeatures: stpy_trsv")           # a hand-off wait that gave up has poisoned z / alpha with NaN
		theta = torch.empty((PhiT.shape[0],), dtype=PhiT.dtype, device=PhiT.device)
		_lib.predict(PhiT, alpha, theta)                                  # theta = Phi^T alpha
		self._factor, self._theta = F, theta
		self.fitted = True

	# ------------------------------------------------------------------ V, V^-1
	def _V_device(self):
		"""The matrix ``self.V`` of the reference: primal Phi^T Phi + s^2 lam I (:239); dual the first-column form of get_invV (:167-170)."""
		c = float(self.s) ** 2 * float(self.lam)
		if self.dual:
			q0 = self._PhiT[:, :1].contiguous()                          # Q^T[:, group = [0]]: the features of the first data point
			m = q0.shape[0]
			V = torch.empty((m, m), dtype=q0.dtype, device=q0.device)
			_lib.gemm_nt(q0, q0, V)
			_lib.combine(V, V, _lib.OUT_SET, c)
			return V
		V = torch.empty_like(self._Vacc)
		_lib.combine(V, self._Vacc, _lib.OUT_SET, c)
		_lib.symmetrize_lower(V)
		return V

	@property
	def V(self):
		"""Phi^T Phi + s^2 lam I (kernelized_features.py:239), full symmetric; built on demand from the accumulated lower tiles."""
		self.precompute()
		return _lib.like_input(self._V_device(), self.x)

	def _invV_device(self):
		if self.dual:
			V = self._V_device()
			L, winv = self._chol(V, "V (dual get_invV)")
			return _lib.potri(L, winv)
		return _lib.potri(self._L, self._winv)                           # a matrix of the caller's own (sample_theta factors it in place)

	@property
	def invV(self):
		"""V^-1 (the reference keeps pinverse(V), kernelized_features.py:240); from the factor on demand."""
		return self.get_invV()

	def get_invV(self):
		"""kernelized_features.py:164-174."""
		self.precompute()
		return _lib.like_input(self._invV_device(), self.x)

	def theta_mean(self, var=False, prior=False):
		"""kernelized_features.py:248-264."""
		self.precompute()
		if self.fitted and not prior:
			theta = _lib.like_input(self._theta.reshape(-1, 1), self.x)
		else:
			theta = 0 * torch.ones(size=(self.get_basis_size(), 1)).double()
		if var is False:
			return theta
		if not (self.fitted and not prior):
			raise UnboundLocalError("theta_mean(var=True) needs a fitted model (the reference leaves Z undefined here, :258-264)")
		if not self.dual:
			Z = float(self.s) ** 2 * self.invV                       # (host-side scale of a returned matrix, as :257)
			return (theta, Z)
		# dual: Z = invK_V = (I - Q^T K^-1 Q) / lam = (I - W W^T) / lam with W = Q^T L^-T  (m x n)
		L = self._L
		m = self._PhiT.shape[0]
		W = self._PhiT.clone()
		_lib.trsm_right_lt(W, L, self._winv, self.nb)
		Z = torch.eye(m, dtype=L.dtype, device=L.device)
		_lib.gemm_nt(W, W, Z, 1)
		if float(self.lam) != 1.0:
			inv_lam = torch.full((m, m), 1.0 / float(self.lam), dtype=L.dtype, device=L.device)
			_lib.combine(Z, inv_lam, _lib.OUT_MUL)
		return (theta, _lib.like_input(Z, self.x))

	# ------------------------------------------------------------------ predict
	def mean(self, xtest):
		return self.mean_std(xtest)[0]

	def mean_std(self, xtest):
		"""kernelized_features.py:269-288.  A test tensor with requires_grad gets a graph (the input gradients of the module header)."""
		if _wants_grad(xtest):
			return _PosteriorFn.apply(self, xtest)
		mu, std, _ = self._posterior(xtest)
		return (_lib.like_input(mu.reshape(-1, 1), xtest), _lib.like_input(std.reshape(-1, 1), xtest))

	def _posterior(self, xtest):
		"""mu, std (M,) on the device and what their input gradient needs: (xt, Phi, std)."""
		self.precompute()
		L, winv, u = self._L, self._winv, self._z
		xt = _lib.to_device(xtest, L.dtype)
		Phi = _lib.to_device(self.embedding.embed(xt), L.dtype)          # (M, m): rows = right-hand sides
		if Phi.stride(1) != 1:
			Phi = Phi.contiguous()
		M = Phi.shape[0]
		mu, ss = torch.empty((M,), dtype=L.dtype, device=L.device), torch.empty((M,), dtype=L.dtype, device=L.device)
		std = torch.empty_like(ss)
		if not self.dual:
			X = Phi.clone()
			_lib.trsm_right_lt(X, L, winv, self.nb)
			_lib.predict(X, u, mu, ss, clamp=2)
			# std = s sqrt(ss) = sqrt(0 - (-s^2) ss): the prediction epilogue with a zero prior term (no torch arithmetic on the vectors)
			_lib.predict_finish(sumsq=ss, kdiag=torch.zeros_like(ss), scale=-float(self.s) ** 2, sigma=std)
			return mu, std, (xt, Phi, std)
		# dual: K* = Phi* Phi^T (M x n), X = K* L^-T, mean = X z, var = (|phi*|^2 - rowsum(X o X)) / lam
		PhiTr = self._PhiT.t().contiguous()                               # (n, m)
		n = PhiTr.shape[0]
		X = torch.empty((M, n), dtype=L.dtype, device=L.device)
		_lib.gemm_nt(Phi, PhiTr, X)
		_lib.trsm_right_lt(X, L, winv, self.nb)
		_lib.predict(X, u, mu, ss, clamp=2)
		kd = torch.empty_like(ss)                                         # |phi*|^2: the same row-sum kernel on Phi*
		_lib.predict(Phi, self._theta, sigma=kd, clamp=2)
		_lib.predict_finish(sumsq=ss, kdiag=kd, scale=1.0, sigma=std, clamp=1 if self.clamp_variance else 0)
		if float(self.lam) != 1.0:                                        # ... / sqrt(lam): the epilogue's scale on a vector
			_lib.predict_finish(mu=std, scale=1.0 / math.sqrt(float(self.lam)))
		return mu, std, (xt, Phi, std)

	mean_var = mean_std

	# ------------------------------------------------------------------ input gradients (kernelized_features.py:441-535)
	def _phi_z(self, Phi):
		"""(Phi Z up to its scalar, the scalar): Z = s^2 V^-1 (primal), (I - Phi_train^T K^-1 Phi_train) / lam (dual).  (M, m)."""
		inv = self._factor.inverse()                                      # V^-1 (primal) / K^-1 (dual): one stpy_potri per fit
		if not self.dual:
			out = torch.empty_like(Phi)
			_lib.gemm_nt(Phi, inv, out)                                   # V^-1 is symmetric: Phi V^-1 = Phi (V^-1)^T
			return out, float(self.s) ** 2
		PhiTr = self._PhiT.t().contiguous()                               # (n, m)
		M, n = Phi.shape[0], PhiTr.shape[0]
		Ks = torch.empty((M, n), dtype=Phi.dtype, device=Phi.device)
		_lib.gemm_nt(Phi, PhiTr, Ks)                                      # K* = Phi* Phi^T
		A = torch.empty_like(Ks)
		_lib.gemm_nt(Ks, inv, A)                                          # K* K^-1
		out = Phi.clone()
		_lib.gemm_nt(A, self._PhiT, out, 1)                               # Phi* - (K* K^-1) Phi_train
		return out, 1.0 / float(self.lam)

	def _posterior_coeffs(self, state, gmu, gstd):
		"""C (M, m) with C_t = gmu_t theta + (gstd_t / sigma_t) Phi_t Z, the sigma part 0 where sigma_t is 0; None when both
		upstream gradients are absent or zero."""
		xt, Phi, std = state
		u = None if gmu is None else _lib.to_device(gmu, xt.dtype).reshape(-1, 1).contiguous()
		gs = None if gstd is None else _lib.to_device(gstd, xt.dtype).reshape(-1)
		if gs is not None and not bool((gs != 0).any()):
			gs = None
		C = None
		if gs is not None:
			C, scal = self._phi_z(Phi)
			pos = std > 0
			v = torch.where(pos, scal * gs / torch.where(pos, std, torch.ones_like(std)), torch.zeros_like(gs))
			C.mul_(v.reshape(-1, 1))                                      # row scaling by the M per-point factors
		if u is not None:
			theta = self._theta.reshape(-1, 1).contiguous()
			if C is None:
				C = torch.empty_like(Phi)
				_lib.gemm_nt(u, theta, C, 0)                              # u theta^T: a K = 1 product
			else:
				_lib.gemm_nt(u, theta, C, 2)
		return C

	def _grad_embedding(self):
		emb = self.embedding
		if not hasattr(emb, "_grad_device"):
			raise NotImplementedError("KernelizedFeatures: input gradients need an embedding with a device description of its feature map "
									  "(RFFEmbedding, the QuadratureEmbedding family, ConcatEmbedding of those); %s has none" % type(emb).__name__)
		return emb

	def _posterior_grad(self, state, gmu, gstd):
		"""sum_t gmu_t grad mu(xt_t) + gstd_t grad sigma(xt_t), one row per test point: (M, d) on the device."""
		xt = state[0]
		C = self._posterior_coeffs(state, gmu, gstd)
		if C is None:
			return torch.zeros(xt.shape, dtype=xt.dtype, device=xt.device)
		G = torch.empty(xt.shape, dtype=xt.dtype, device=xt.device)
		self._grad_embedding()._grad_device(xt, C, G)
		return G

	def _value_grad(self, xt, theta_row, hessian=False):
		"""Batched phi(x_t)^T theta with its gradient (and Hessian) for ONE coefficient row shared by all points: (val (M,),
		G (M, d)[, H (M, d, d)]) on the device from one launch."""
		xt = _lib.to_device(xt, theta_row.dtype)
		return self._grad_embedding().value_grad(xt, theta_row, hessian=hessian)

	def _mean_hessian(self, xtest):
		"""Gradient (M, d) and Hessian (M, d, d) of the posterior mean at every row of xtest (the order-2 path of stpy_rff_grad; the
		reference's mean_gradient_hessian(x, hessian=True), :441-456, is row 0 of this)."""
		self.precompute()
		_, G, H = self._value_grad(_lib.to_device(xtest, self._L.dtype), self._theta.reshape(-1).contiguous(), hessian=True)
		return _lib.like_input(G, xtest), _lib.like_input(H, xtest)

	def sample_and_optimize(self, xtest=None, multistart=25, minimizer="L-BFGS-B", grid=100, verbose=0):
		"""
		kernelized_features.py:501-535: draw theta (the reference's draw first, so a seeded run sees the same theta), then maximise
		f(x) = phi(x)^T theta over ``self.bounds`` (or (-diameter, diameter)^d) from ``multistart`` uniform starts drawn with the
		reference's np.random calls in its order.  First order: every step is one stpy_rff_grad launch with the shared row theta
		that returns the values and gradients of all starts together.  Returns (solution (d,), value (1,)) of the best start.
		"""
		thT = self._sample_theta_t()                                       # (1, basis), device
		if self.bounds is None:
			mybounds = tuple([(-self.diameter, self.diameter) for _ in range(self.d)])
		else:
			mybounds = self.bounds
		if minimizer != "L-BFGS-B":
			raise AssertionError("Wrong optimizer selected.")
		starts = _draw_starts(multistart, self.d, mybounds)
		row = thT.reshape(-1).contiguous()
		sol, vals, evals = _multistart_maximize(lambda xt: self._value_grad(xt, row), starts, mybounds, _lib.device(), row.dtype)
		self._last_optimize_evaluations = evals
		if verbose:
			print("sample_and_optimize: %d starts, %d device evaluations" % (len(starts), evals))
		index = int(np.argmax(vals))
		return (torch.from_numpy(sol[index].copy()), torch.from_numpy(vals[index:index + 1].copy()))

	# These four names of GaussianProcess stay refused for now: the machinery above serves them (``_posterior_grad`` is mean_std_grad,
	# ``_mean_hessian`` is mean_gradient_hessian, gauss_procc's ``_multistart_maximize`` with ``_posterior`` + ``_posterior_grad`` is ucb_optimize),
	# and the inherited methods would differentiate the kernel-space posterior, i.e. return numbers of the wrong model.
	def _no_input_gradients(self, *args, **kwargs):
		raise NotImplementedError("KernelizedFeatures does not expose mean_std_grad, mean_gradient_hessian, gradient_mean_var and ucb_optimize "
								  "(the GaussianProcess methods differentiate the kernel, not the embedding); its input gradients are "
								  "reached by autograd through mean_std / mean_var / mean / ucb / lcb on a test tensor with requires_grad, "
								  "and by sample_and_optimize")

	mean_std_grad = mean_gradient_hessian = gradient_mean_var = ucb_optimize = _no_input_gradients

	def ucb(self, xtest, delta=0.1):
		mu, std = self.mean_std(xtest)
		return mu + np.sqrt(self.beta(delta=delta)) * std

	def lcb(self, xtest, delta=0.1):
		mu, std = self.mean_std(xtest)
		return mu - np.sqrt(self.beta(delta=delta)) * std

	def residuals(self):
		"""kernelized_features.py:559-562: sum (mean(x) - y)^2."""
		mu, _ = self.mean_std(self.x)
		r = _lib.to_device(mu).reshape(-1, 1).clone()
		y = _lib.to_device(self.y, r.dtype).reshape(-1, 1).contiguous()
		one = torch.ones((1, 1), dtype=r.dtype, device=r.device)
		# r -= y 1^T (a K = 1 product in the subtracting mode), then <r, r>
		_lib.gemm_nt(y, one, r, 1)
		return _lib.like_input(_lib.trace_dot(u=r, v=r)[1].reshape(()).clone(), self.x)

	# ------------------------------------------------------------------ sampling
	def _draw(self, basis, size):
		"""The reference's draw (kernelized_features.py:302-303, :323-324): CPU generator, (basis, size) standard normals."""
		zeros = torch.zeros(size=(basis, size), dtype=torch.float64)
		return torch.normal(mean=zeros, std=1.)

	def _prior_theta_t(self, random_vector, dtype, device):
		"""theta^T (size, basis) of the prior branch: chol(lam I) r + prior_mean = sqrt(lam) r + prior_mean (:305-307, :332-334).
		The scaling is applied to the host-side draw before it is uploaded."""
		th = math.sqrt(float(self.lam)) * random_vector
		if torch.is_tensor(self.prior_mean) or self.prior_mean != 0:
			th = th + self.prior_mean
		return th.T.contiguous().to(device=device, dtype=dtype)

	def _sample_theta_t(self, size=1, prior=False):
		"""theta^T on the device, (size, basis)."""
		basis = self.get_basis_size()
		random_vector = self._draw(basis, size)
		self.precompute()
		if not (self.fitted == True and prior == False):
			dev = _lib.device()
			dtype = self._L.dtype if self._L is not None else torch.float64
			return self._prior_theta_t(random_vector, dtype, dev)
		# L = chol(get_invV()) * s, theta = theta_mean + L r  (:328-330).  theta^T = 1 theta_mean^T + (s r)^T L^T: the accumulating
		# NT product of the scaled draw (size x basis) with the lower-triangular factor
		# (the factor of V^-1 is kept with the resident factor of V: potri -> potrf -> tril once per fit, downdated by a one-row update)
		F = self._factor
		if F._sampler is None:
			Lc, winvc = self._chol(self._invV_device(), "V^-1 (sample_theta)")
			_lib.tril(Lc)
			F._sampler = (Lc, winvc)
		Lc = F._sampler[0]
		rt = (float(self.s) * random_vector).T.contiguous().to(device=Lc.device, dtype=Lc.dtype)          # (size, basis)
		thT = torch.empty((size, basis), dtype=Lc.dtype, device=Lc.device)
		thT.copy_(self._theta.reshape(1, basis).expand(size, basis))
		_lib.gemm_nt(rt, Lc, thT, 2)
		return thT

	def sample_theta(self, size=1, prior=False):
		"""kernelized_features.py:319-336: (basis, size)."""
		thT = self._sample_theta_t(size=size, prior=prior)
		return _lib.like_input(thT.t(), self.x if self.x is not None else torch.zeros(1))

	def _features_times_theta(self, xtest, thT, out=None, mode=0):
		"""Phi(xtest) theta, (M, size), device (``out`` given: accumulated per ``mode``)."""
		xt = _lib.to_device(xtest, thT.dtype)
		Phi = _lib.to_device(self.embedding.embed(xt), thT.dtype)
		if Phi.stride(1) != 1:
			Phi = Phi.contiguous()
		if out is None:
			out = torch.empty((Phi.shape[0], thT.shape[0]), dtype=thT.dtype, device=thT.device)
		_lib.gemm_nt(Phi, thT, out, mode)
		return out

	def sample(self, xtest, size=1, prior=False):
		"""kernelized_features.py:537-543: Phi(xtest) theta for a sampled theta, (M, size)."""
		thT = self._sample_theta_t(size=size, prior=prior)
		return _lib.like_input(self._features_times_theta(xtest, thT), xtest)

	def sample_and_max(self, xtest, size=1):
		"""kernelized_features.py:545-551."""
		f = self.sample(xtest, size=size)
		index = torch.argmax(f, dim=0)
		return (xtest[index, :], f[index, :])

	def sample_matheron(self, xtest, kernel_object, size=1):
		"""
		kernelized_features.py:300-317 (pathwise / Matheron update): a prior draw in feature space, corrected by the exact GP of
		``kernel_object`` on the data:  f = Phi* theta + K* (K + s^2 lam I)^-1 (y - Phi theta).
		"""
		basis = self.get_basis_size()
		random_vector = self._draw(basis, size)
		xd = _lib.to_device(self.x)
		dtype, dev = xd.dtype, xd.device
		thT = self._prior_theta_t(random_vector, dtype, dev)                                    # (size, basis)
		xt = _lib.to_device(xtest, dtype)
		N, M = xd.shape[0], xt.shape[0]
		f = self._features_times_theta(xt, thT)                                                 # f_prior_xtest (M, size)
		# R^T = 1 y^T - theta^T Phi^T  (size, N): the residual of the prior draw on the data, rows = right-hand sides
		Rt = torch.empty((size, N), dtype=dtype, device=dev)
		Rt.copy_(_lib.to_device(self.y, dtype).reshape(1, N).expand(size, N))
		Phi = _lib.to_device(self.embedding.embed(xd), dtype)
		if Phi.stride(1) != 1:
			Phi = Phi.contiguous()
		_lib.gemm_nt(thT, Phi, Rt, 1)
		del Phi
		# K = k(x, x) + s^2 lam I -> Cholesky;  f += (K* L^-T) (R^T L^-T)^T
		K = torch.empty((N, N), dtype=dtype, device=dev)
		kernel_object._kernel_into(xd, xd, K, None, diag_add=float(self.s) ** 2 * float(self.lam), lower_only=True)
		L, winv = self._chol(K, "k(x, x) + s^2 lam I (sample_matheron)")
		_lib.trsm_right_lt(Rt, L, winv, self.nb)
		X = torch.empty((M, N), dtype=dtype, device=dev)
		kernel_object._kernel_into(xd, xt, X)                                                   # K* = k(x, xtest): (M, N)
		_lib.trsm_right_lt(X, L, winv, self.nb)
		_lib.gemm_nt(X, Rt, f, 2)
		return _lib.like_input(f, xtest)
