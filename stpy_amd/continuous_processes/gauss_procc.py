"""
Drop-in for ``stpy.continuous_processes.gauss_procc.GaussianProcess`` on the squared-loss path
(reference: stpy/continuous_processes/gauss_procc.py:18-71 ctor, :100-117 add_data_point / fit,
:136-177 fit_gp, :198-209 execute, :310-418 mean_std / mean, :497-504 + :631-638 log_marginal,
:915 get_kernel; explicit-Cholesky form of the evidence in stpy/estimator.py:32-40).

What runs where
  Gram matrices      stpy_gram              (csrc/gram.hip)
  K = L L^T          stpy_potrf             (csrc/potrf.hip + csrc/gemm.hip, fp64/fp32 MFMA)
  z = L^-1 y, alpha  stpy_trsv              (csrc/solve.hip)
  X = K* L^-T        stpy_trsm_right_lt     (csrc/solve.hip + csrc/gemm.hip)
  mu, sigma          stpy_predict           (csrc/solve.hip)
  log det, y^T K^-1 y  stpy_logdet_quad     (csrc/solve.hip)
  d mu, d sigma / dx*  stpy_gram_grad, stpy_trsm_right_ln   (csrc/grad.hip)
Python only sequences those calls and owns the torch tensors they operate on.

The reference solves with lstsq / LU / slogdet; an SPD solve through the Cholesky factor is the
same mathematics (and what Estimator.log_marginal does), agreement is checked to <= 1e-8 relative
against golden vectors captured from the reference (tests/golden).

Differences a caller can observe, all deliberate:
  * ``self.K`` / ``self.Sigma`` are materialised lazily (the factorisation is in place; at
    N = 65 536 a second N x N matrix is 34 GB); ``self.B`` (N x N, a by-product of the reference's
    lstsq, gauss_procc.py:378) is not kept.
  * prediction before ``fit`` with ``full=False`` returns the prior (0, sqrt(diag K**)) that
    gauss_procc.py:349-363 intends; the reference snapshot raises TypeError there (:346).
  * ``add_data`` / ``mean_var`` are aliases of ``add_data_point`` / ``mean_std`` (the names used in
    BASELINE.json); like every ``mean_var`` in stpy they return (mean, *std*).
  * robust losses, sampling helpers, gradients, UCB optimisation are outside the hot path.
"""
import numpy as np
import math
import operator

import torch

from .. import _lib
from ..estimator import Estimator
from ..kernels import KernelFunction


_GRAD_NAMES = ("gamma", "ard_gamma", "cov")          # what the dense evidence differentiates: lengthscales and the map of a full-covariance item


class _LogMarginalFn(torch.autograd.Function):
	"""Autograd node of GaussianProcess.log_marginal: forward = the HIP evidence, backward = its analytic gradient."""

	@staticmethod
	def forward(ctx, gp, kernel, X, weight, *tensors):
		val, state = gp._log_marginal_value(kernel, X, weight)
		ctx.gp, ctx.kernel, ctx.X, ctx.weight, ctx.state = gp, kernel, X, weight, state
		ctx.params = gp._grad_params(X, _GRAD_NAMES)
		return val.clone()

	@staticmethod
	def backward(ctx, gout):
		grads = ctx.gp._log_marginal_grads(ctx.kernel, ctx.X, ctx.weight, ctx.state, ctx.params)
		scale = gout.reshape(-1)[0]
		return (None, None, None, None) + tuple(scale.to(g.device) * g for g in grads)


class _PosteriorFn(torch.autograd.Function):
	"""Autograd node of ``mean_std`` for a test tensor with requires_grad, for any owner with ``_posterior(xtest) -> (mu, sigma, state)``
	(device vectors) and ``_posterior_grad(state, gmu, gstd) -> (M, d)``: forward = the HIP prediction, backward = the owner's input
	gradient (GaussianProcess: one stpy_gram_grad launch per kernel term; KernelizedFeatures: one stpy_rff_grad launch)."""

	@staticmethod
	def forward(ctx, gp, xtest):
		ctx.set_materialize_grads(False)
		mu, sigma, state = gp._posterior(xtest.detach())
		ctx.gp, ctx.state, ctx.like = gp, state, (xtest.device, xtest.dtype, tuple(xtest.shape))
		return _lib.like_input(mu.reshape(-1, 1), xtest), _lib.like_input(sigma.reshape(-1, 1), xtest)

	@staticmethod
	def backward(ctx, gmu, gstd):
		dev, dt, shape = ctx.like
		g = ctx.gp._posterior_grad(ctx.state, gmu, gstd)
		return None, g.to(device=dev, dtype=dt).reshape(shape)


class _MeanFn(torch.autograd.Function):
	"""Autograd node of GaussianProcess.mean (K* alpha): backward = stpy_gram_grad with u = g_mu on alpha."""

	@staticmethod
	def forward(ctx, gp, xtest):
		ctx.gp, ctx.like = gp, (xtest.device, xtest.dtype, tuple(xtest.shape))
		ctx.xt = _lib.to_device(xtest.detach(), gp._xd.dtype)
		return gp._mean_value(xtest.detach())

	@staticmethod
	def backward(ctx, gmu):
		dev, dt, shape = ctx.like
		gp = ctx.gp
		G = torch.zeros(ctx.xt.shape, dtype=ctx.xt.dtype, device=ctx.xt.device)
		u = _lib.to_device(gmu, ctx.xt.dtype).reshape(-1).contiguous()
		gp.kernel_object._grad_into(gp._xd, ctx.xt, G, alpha=gp._alpha.reshape(-1).contiguous(), u=u)
		return None, G.to(device=dev, dtype=dt).reshape(shape)


def _wants_grad(xtest):
	return torch.is_tensor(xtest) and xtest.requires_grad and torch.is_grad_enabled()


def _weight(weight):
	"""The evidence's log-det weight as a host float (a python number or a one-element tensor)."""
	return float(weight.item()) if torch.is_tensor(weight) else float(weight)


def _tile_pad(n):
	"""Order at which an n x n SPD matrix is held on the device: the next multiple of the 128 x 128 GEMM tile."""
	return -(-int(n) // 128) * 128


def _draw_starts(multistart, d, bounds):
	"""``multistart`` uniform starts in the box ``bounds``, drawn with the reference's np.random calls in its order (randn(d), then d
	uniforms, per start: gauss_procc.py:935-938, kernelized_features.py:515-518), so a seeded run starts where the reference does."""
	starts = []
	for _ in range(multistart):
		x0 = np.random.randn(d)
		for i in range(d):
			x0[i] = np.random.uniform(bounds[i][0], bounds[i][1])
		starts.append(x0)
	return starts


def _multistart_maximize(evaluate, starts, bounds, dev, dtype, final=None):
	"""All starts as ONE L-BFGS-B problem over the stacked points (the objective is a sum of independent terms): ``evaluate`` maps
	device points (S, d) to (values (S,), gradients (S, d)), one batched device evaluation per step.  ``final`` maps the solution to
	its values alone, for a caller whose values come cheaper without gradients (default: those of ``evaluate``).  Returns (solutions
	(S, d), values (S,), number of evaluations, the final one included) as NumPy float64."""
	from scipy.optimize import minimize
	S, d = len(starts), len(starts[0])
	count = [0]

	def at(z, f):
		count[0] += 1
		return f(torch.from_numpy(np.ascontiguousarray(z.reshape(S, d))).to(device=dev, dtype=dtype))

	def fun(z):
		val, g = at(z, evaluate)
		return -float(val.sum().item()), -g.double().cpu().numpy().reshape(-1)

	res = minimize(fun, np.concatenate(starts), method="L-BFGS-B", jac=True, bounds=list(bounds) * S,
				   options=dict(maxiter=15000, ftol=1e-15, gtol=1e-10))
	vals = at(res.x, final or (lambda xt: evaluate(xt)[0]))
	return res.x.reshape(S, d), vals.double().cpu().numpy(), count[0]


def normalize_remove_index(index, n):
	"""The rows ``remove_data_point`` is asked to drop from n points, as a sorted list of distinct ints in [0, n).  ``index``: an int, a
	sequence of ints or a 1-D integer tensor / array; negative values count from the end.  IndexError for a value outside [-n, n),
	ValueError for a repeated row (after the negative ones are resolved), TypeError for anything that is not an integer."""
	if torch.is_tensor(index) or isinstance(index, np.ndarray):
		if index.ndim > 1:
			raise ValueError("remove_data_point: index must be an int or one-dimensional, got shape %s" % (tuple(index.shape),))
		if torch.is_tensor(index) and (index.dtype.is_floating_point or index.dtype.is_complex or index.dtype == torch.bool):
			raise TypeError("remove_data_point: index tensor of dtype %s (integers expected)" % index.dtype)
		vals = index.reshape(-1).tolist()
	elif isinstance(index, (list, tuple, range)):
		vals = list(index)
	else:
		vals = [index]
	out = []
	for v in vals:
		if isinstance(v, bool):
			raise TypeError("remove_data_point: index %r is not an integer" % (v,))
		try:
			v = operator.index(v)
		except TypeError:
			raise TypeError("remove_data_point: index %r is not an integer" % (v,))
		if v < -n or v >= n:
			raise IndexError("remove_data_point: index %d is out of range for %d points" % (v, n))
		out.append(v + n if v < 0 else v)
	out.sort()
	for a, b in zip(out, out[1:]):
		if a == b:
			raise ValueError("remove_data_point: row %d is listed more than once" % a)
	return out


class ResidentFactor:
	"""The Cholesky factor of one (data, hyper-parameters) pair on the device, and what is derived from it at most once.  An estimator
	holds it in ``_factor`` and drops all of it with ``_factor = None``.
	  L, winv   the factor (GaussianProcess: tile-padded, lower triangle) and the inverse 128 x 128 diagonal blocks of stpy_potrf
	  n         order of the matrix that was factored (L's order without the padding)
	  buf       the capacity buffer L is a leading view of after an append (room for more rows), else None
	  z         L^-1 y; None on a factor nobody solved with
	  key       GaussianProcess._hyper_key of the hyper-parameters it was built from, None where nothing compares it
	An estimator that modifies L in place (KernelizedFeatures: stpy_chol_update) resets the derived fields itself; ``_sampler`` is its
	(chol((L L^T)^-1), inverse diagonal blocks) pair for the theta draws, None until the first draw."""

	def __init__(self, L, winv, n=None, z=None, key=None, buf=None):
		self.L, self.winv, self.n, self.z, self.key, self.buf = L, winv, L.shape[0] if n is None else n, z, key, buf
		self._alpha = self._reversed = self._inverse = self._sampler = None

	def solve(self, y):
		"""z = L^-1 y, kept; returns alpha = L^-T z."""
		self.z, self._alpha = _lib.trsv(self.L, self.winv, y), None
		return self.alpha

	@property
	def alpha(self):
		"""K^-1 y = L^-T z, (n,)."""
		if self._alpha is None:
			self._alpha = _lib.trsv(self.L, self.winv, self.z, trans=1)[:self.n]
		return self._alpha

	def reversed(self):
		"""(J L^T J, its inverse diagonal blocks) for B L^-1 (stpy_trsm_ln_factor): another matrix of L's size."""
		if self._reversed is None:
			self._reversed = _lib.trsm_ln_factor(self.L, self.winv)
		return self._reversed

	def inverse(self):
		"""(L L^T)^-1, full symmetric (stpy_potri): read-only for its users."""
		if self._inverse is None:
			self._inverse = _lib.potri(self.L, self.winv)
		return self._inverse


def _of_factor(name):
	"""Read-only estimator property: that field of the resident factor, None without a factor."""
	return property(lambda self: None if self._factor is None else getattr(self._factor, name))


class GaussianProcess(Estimator):

	def __init__(self, gamma=1, s=0.001, kappa=1., kernel_name="squared_exponential", diameter=1.0,
				 groups=None, bounds=None, nu=1.5, kernel=None, d=1, power=2, lam=1., loss='squared', huber_delta=1.35,
				 hyper='classical', B=1., svr_eps=0.1):
		if loss != 'squared':
			raise NotImplementedError("loss='%s': only the squared loss is on the stpy_amd hot path "
									  "(huber/svr/unif need cvxpy/MOSEK, gauss_procc.py:211-308)" % loss)
		self.s = s
		self.d = d
		self.x = None
		self.y = None
		self.n = 0
		self.mu = 0.0
		self.lam = lam
		self.total_bound = B
		self.safe = False
		self.fitted = False
		self.diameter = diameter
		self.bounds = bounds
		self.admits_first_order = False
		self.back_prop = True
		self.loss = loss
		self.hyper = hyper
		self.max_size = 10000               # gauss_procc.py:55: prediction chunk
		self.clamp_variance = False         # the reference takes sqrt of the raw difference (:394-395)
		self.nb = 0                         # outer panel width for potrf/trsm (0 = library default)
		self.delete_max_rank = 128          # remove_data_point(iterative=True): more rows than this are refitted (each costs a rotation pass)
		self.remove_path = None             # which route the last remove_data_point took: "update" or "refit"
		if kernel is not None:
			self.kernel_object = kernel
			self.kernel = kernel.kernel
			self.d = kernel.d
		else:
			self.kernel_object = KernelFunction(kernel_name=kernel_name, gamma=gamma, nu=nu, groups=groups, kappa=kappa,
												power=power, d=d)
			self.kernel = self.kernel_object.kernel
			self.gamma = gamma
			self.v = nu
			self.groups = groups
			self.kappa = kappa
			self.custom = kernel
			self.optkernel = kernel_name
		# device state
		self._xd = None
		self._yd = None
		self._Sigma = None
		self._factor = None     # ResidentFactor of k(x,x) + Sigma^T Sigma; ``fitted`` implies there is one

	_L, _winv, _z, _alpha, _Lbuf = (_of_factor(name) for name in ("L", "winv", "z", "alpha", "buf"))

	# ------------------------------------------------------------------ small API mirrors
	def description(self):
		return self.kernel_object.description() + "\nlambda=" + str(self.s)

	def embed(self, x):
		return self.kernel_object.embed(x)

	def get_basis_size(self):
		return self.kernel_object.get_basis_size()

	def residuals(self, x, y):
		return self.mean(x) - y

	def add_data_point(self, x, y, Sigma=None, iterative=False):
		"""gauss_procc.py:100-111: concatenate and refit from scratch.  ``iterative=True`` extends the resident factor by the new rows
		instead (stpy_potrf_append: one pass over L for a handful of points) whenever that is the same mathematics -- same kernel
		parameters and noise as the factor, no explicit Sigma -- and refits otherwise."""
		if iterative and self.x is not None and Sigma is None and self._Sigma is None:
			self.fit_gp(x, y, iterative=True, extrapoint=True)
			return
		if self.x is not None:
			self.x = torch.cat((self.x, x), dim=0)
			self.y = torch.cat((self.y, y), dim=0)
			if Sigma is None and self._Sigma is not None:
				self._Sigma = torch.block_diag(self._Sigma, torch.eye(x.size()[0], dtype=torch.double) * self.s)
		else:
			self.x = x
			self.y = y
			self._Sigma = Sigma
		self.fit_gp(self.x, self.y, Sigma=self._Sigma)

	add_data = add_data_point

	def remove_data_point(self, index, iterative=False):
		"""Forget observations: ``index`` names rows of x / y (an int, a sequence of ints or a 1-D integer tensor; negative values count from
		the end).  The default mirrors ``add_data_point``: slice the data and refit; a resident explicit Sigma is kept as Sigma[R][:, R]
		when it is diagonal (the only form add_data_point builds), anything else is refused so that the caller refits explicitly.
		``iterative=True`` deletes the rows from the resident factor instead (stpy_potrf_delete: a gather and, per 32 rows, one pass over
		the part of L below the first deleted row) whenever that is the same mathematics -- the conditions of the append, and at most
		``delete_max_rank`` rows -- and refits otherwise.  ``self.remove_path`` tells which ran ("update" / "refit").
		IndexError: a row out of range; ValueError: a repeated row, every row, an unfitted or empty GP.  A refused call changes nothing."""
		if not self.fitted or self.x is None or self.n == 0 or self._factor is None:
			raise ValueError("remove_data_point: the GP holds no fitted data")
		idx = normalize_remove_index(index, self.n)
		if len(idx) == 0:
			return
		if len(idx) >= self.n:
			raise ValueError("remove_data_point: cannot remove all %d points" % self.n)
		Sigma = self._Sigma
		if Sigma is not None:
			Sigma = torch.as_tensor(Sigma)
			if Sigma.dim() != 2 or Sigma.shape[0] != self.n or Sigma.shape[1] != self.n or not torch.equal(Sigma, torch.diag(torch.diagonal(Sigma))):
				raise ValueError("remove_data_point: the explicit Sigma is not diagonal; slice the data and call fit_gp with the Sigma of the kept rows")
		mask = torch.ones((self.n,), dtype=torch.bool)
		mask[idx] = False
		keep = mask.nonzero().reshape(-1)
		n0 = self.n
		if iterative and 1 <= len(idx) <= self.delete_max_rank and self._can_append(self.x, None):
			if self._delete(idx, keep):
				self.remove_path = "update"
				return
		x, y = self.x, self.y
		if self.n == n0:                  # (else _delete has sliced them already: its factor was not good, or the hand-off of a solve gave up)
			x, y = x[keep.to(x.device)], y[keep.to(y.device)]
			if Sigma is not None:
				ks = keep.to(Sigma.device)
				Sigma = Sigma[ks][:, ks]
		self.fit_gp(x, y, Sigma=Sigma)
		self.remove_path = "refit"

	remove_data = remove_data_point

	def fit(self, x=None, y=None):
		"""gauss_procc.py:113-117."""
		if x is not None:
			self.fit_gp(x, y)
		else:
			self.fit_gp(self.x, self.y)

	def lcb(self, xtest):
		mu, s = self.mean_std(xtest)
		return mu - 2 * s

	def ucb(self, xtest):
		mu, s = self.mean_std(xtest)
		return mu + 2 * s

	# ------------------------------------------------------------------ factorisation
	@staticmethod
	def _add_noise_gram(K, Sigma):
		"""K += Sigma^T Sigma = K - (-Sigma^T)(Sigma^T)^T: one stpy_gemm_nt in subtract mode."""
		St = _lib.to_device(Sigma, K.dtype).t().contiguous()
		_lib.gemm_nt(-St, St, K, 1)

	@staticmethod
	def _check_info(info, what="stpy_potrf: the leading minor of order %d of K + s^2 I is not positive definite"):
		"""The one synchronisation of a fit: the factorisation's status word (first failing pivot, 1-based; 0 = fine).  ``what``: the
		message of the LinAlgError raised for a failing pivot, with a %d for its order."""
		bad = int(info.item())
		if bad != 0:
			raise torch.linalg.LinAlgError(what % bad)

	def _factorize(self, kernel, xd, kwargs=None, Sigma=None):
		"""K_theta = k(x,x) + s^2 I (or + Sigma^T Sigma) of ``kernel`` -> in-place Cholesky.  Returns (ResidentFactor, the device
		status word, unread): the caller enqueues what follows the factorisation first and then calls ``_check_info``, so the
		device does not idle through the host round trip."""
		n0 = xd.shape[0]
		n = _tile_pad(n0)
		# The matrix is held at the next multiple of the 128-tile, bordered by an identity block:
		# chol([[K, 0], [0, I]]) = [[L, 0], [0, I]], so every product of the factorisation and of the
		# solves below runs on the tile-aligned kernels whatever N is (a ragged N = 32 700 cost 30 %).
		# Padded entries of y, z, alpha and the padded columns of K* are zero and drop out of every sum.
		Kp = torch.empty((n, n), dtype=xd.dtype, device=xd.device)
		K = Kp[:n0, :n0]
		if n > n0:
			Kp[n0:, :].zero_()
			Kp[:n0, n0:].zero_()              # (upper part of the last diagonal tile: the diagonal-block kernel loads whole tiles)
			Kp[n0:, n0:].diagonal().fill_(1.0)
		if Sigma is None:
			kernel._kernel_into(xd, xd, K, kwargs, diag_add=float(self.s) ** 2, lower_only=True)
		else:
			# general noise matrix (gauss_procc.py:163): K += Sigma^T Sigma through the NT product
			kernel._kernel_into(xd, xd, K, kwargs)
			self._add_noise_gram(K, Sigma)
		winv, info = _lib.potrf(Kp, self.nb)
		return ResidentFactor(Kp, winv, n0), info

	@property
	def A(self):
		"""K^-1 y, (N, 1)  (gauss_procc.py:376)."""
		a = self._alpha
		return None if a is None else _lib.like_input(a.reshape(-1, 1), self.x)

	def fit_gp(self, x, y, Sigma=None, iterative=False, extrapoint=False):
		"""gauss_procc.py:136-177.  ``extrapoint=True``: x, y are only the points to add to the fitted data; otherwise they are all of
		it.  ``iterative=True``: the rows beyond the fitted ones extend the resident factor (bordered Cholesky, stpy_potrf_append)
		instead of refactoring -- taken only when the factor was built with the current noise level and kernel parameters, without
		an explicit Sigma, in the same dtype; anything else (an unfitted GP included) is the ordinary fit on all the data."""
		if extrapoint and self.x is not None:
			x, xn = torch.cat((self.x, x), dim=0), x
			y, yn = torch.cat((self.y, y), dim=0), y
		else:
			xn, yn = x[self.n:], y[self.n:]
		if iterative and xn.shape[0] > 0 and self._can_append(x, Sigma):
			if self._append(x, y, xn, yn):
				return None
		self.n, self.d = x.shape
		self.x = x
		self.y = y
		self._Sigma = Sigma
		self._xd = _lib.to_device(x)
		self._yd = _lib.to_device(y, self._xd.dtype).reshape(-1, 1)
		# not fitted until the new factor exists: a refit that fails (not positive definite, out of memory) leaves an
		# object that takes the prior branch instead of one that reports fitted=True with no factor behind it
		self.fitted = False
		self._factor = None                                             # release the previous factor before allocating the next
		F, info = self._factorize(self.kernel_object, self._xd, None, Sigma)
		# A = K^-1 y is part of the fitted state the reference leaves behind (gauss_procc.py:376): computed
		# eagerly even though mean_std itself only needs z
		F.solve(self._yd)
		# the two vector solves are already queued behind the factorisation when the host reads its status (on a matrix that is
		# not positive definite they ran on garbage and are dropped with the exception: the object stays unfitted)
		self._check_info(info)
		# ... and the sticky device word of the one-launch vector solves: a hand-off wait that gave up has poisoned z / alpha
		# with NaN (stpy_async_status; the stream is already drained by the read above, so this costs one 4-byte copy)
		_lib.check_async("fit_gp: stpy_trsv")
		F.key = self._hyper_key(self.kernel_object)
		self._factor = F
		self.fitted = True
		return None

	def _can_append(self, x, Sigma):
		"""The bordered update computes what a refit would: the factor exists and was built from the current s / kernel parameters
		with the s^2 I noise, and the new points come in its dtype."""
		return (self.fitted and self._factor is not None and Sigma is None and self._Sigma is None
				and self._factor.key == self._hyper_key(self.kernel_object)
				and (x.dtype if torch.is_tensor(x) and x.dtype in (torch.float32, torch.float64) else torch.float64) == self._xd.dtype
				and x.shape[1] == self._xd.shape[1])

	def _append(self, x, y, xn, yn):
		"""Extend the resident factor by the rows xn (x, y: all the data afterwards).  The factor lives in a buffer of capacity cap >= the
		padded order (``_L`` is its leading view, leading dimension cap): appends that fit are in place; a full buffer is replaced by one
		with a tile of headroom, so single-point appends copy the factor at most once per 128 points.  Returns False (the caller refits)
		when that allocation fails."""
		dtype, dev = self._xd.dtype, self._xd.device
		xd_new = _lib.to_device(xn, dtype)
		yd_new = _lib.to_device(yn, dtype).reshape(-1).contiguous()
		n0, k = self.n, xd_new.shape[0]
		n1 = n0 + k
		n1p = _tile_pad(n1)
		buf = self._L if self._Lbuf is None else self._Lbuf
		winv, key = self._winv, self._factor.key
		if n1p > buf.shape[0]:
			n0p = self._L.shape[0]
			cap = n1p + 128
			try:
				nbuf = torch.zeros((cap, cap), dtype=dtype, device=dev)
				nwinv = torch.empty((_lib.potrf_winv_elems(cap),), dtype=dtype, device=dev)
			except RuntimeError:
				nbuf = nwinv = None
				self.fitted = False
				self._factor = None
				return False
			nbuf[:n0p, :n0p].copy_(self._L)
			nwinv[:_lib.potrf_winv_elems(n0p)].copy_(winv[:_lib.potrf_winv_elems(n0p)])
			buf, winv = nbuf, nwinv
		# the new rows of K + s^2 I straight into the factor's buffer, as ONE launch against all the points: the norm-expansion routes
		# of stpy_gram expand about the first row of `a`, and with a = [x_old; x_new] that is x_0 -- the point a fit on all the data
		# expands about -- so every entry comes out bit for bit as a refit would compute it (two launches, one of them with a = x_new,
		# gave the new diagonal block other roundings, which an ill-conditioned fp32 factor amplifies)
		xd_all = torch.cat((self._xd, xd_new), dim=0)
		self.kernel_object._kernel_into(xd_all, xd_new, buf[n0:n1, :n1])
		_lib.combine(buf[n0:n1, n0:n1], buf[n0:n1, n0:n1], _lib.OUT_SET, float(self.s) ** 2)
		z = torch.zeros((n1p,), dtype=dtype, device=dev)
		z[:n0] = self._z[:n0]
		# from here on the object describes the new data set, fitted only once the extended factor is known to be good (the rows just
		# written into the buffer overwrote the identity padding of the old factor)
		self.x, self.y, self.n = x, y, n1
		self._xd = xd_all
		self._yd = torch.cat((self._yd, yd_new.reshape(-1, 1)), dim=0)
		self.fitted = False
		self._factor = None
		info = _lib.potrf_append(buf, n0, winv, z, yd_new)
		self._check_info(info)
		_lib.check_async("add_data_point: stpy_potrf_append")
		self._factor = ResidentFactor(buf[:n1p, :n1p], winv, n1, z=z, key=key, buf=buf)
		self.fitted = True
		return True

	def _delete(self, idx, keep):
		"""Drop the rows ``idx`` (sorted; ``keep``: the others, a long tensor) from the resident factor.  The compaction is out of place: the
		new factor goes into a fresh buffer of the SAME capacity as the one it replaces, so that later appends stay in place.  Returns
		False when the caller has to refit: before anything changed if that allocation fails, with x / y already sliced if the status
		word or the solves' hand-off word is set."""
		dtype, dev = self._xd.dtype, self._xd.device
		old = self._factor
		n0, n1 = self.n, self.n - len(idx)
		n1p = _tile_pad(n1)
		cap = (old.L if old.buf is None else old.buf).shape[0]
		try:
			nbuf = torch.zeros((cap, cap), dtype=dtype, device=dev)
			nwinv = torch.empty((_lib.potrf_winv_elems(cap),), dtype=dtype, device=dev)
		except RuntimeError:
			nbuf = nwinv = None
			return False
		info = _lib.potrf_delete(old.L, n0, idx, nbuf, nwinv)
		kd = keep.to(dev)
		self.x, self.y, self.n = self.x[keep.to(self.x.device)], self.y[keep.to(self.y.device)], n1
		self._xd, self._yd = self._xd[kd], self._yd[kd]
		self.fitted = False
		self._factor = None
		F = ResidentFactor(nbuf[:n1p, :n1p], nwinv, n1, key=old.key, buf=nbuf)
		F.solve(self._yd)                                                  # A = K^-1 y is part of the fitted state: two vector solves
		ok = int(info.item()) == 0
		try:
			_lib.check_async("remove_data_point: stpy_trsv")
		except _lib.StpyHipError:
			ok = False
		if not ok:
			return False
		self._factor = F
		self.fitted = True
		return True

	def _hyper_key(self, kernel):
		"""What the resident factor was built from: the noise level and every stored kernel parameter, by value.
		log_marginal re-uses the factor only while this is unchanged (the reference rebuilds K from the CURRENT
		self.s / params_dict on every call, gauss_procc.py:631-638)."""
		def freeze(v):
			if torch.is_tensor(v):
				return ("t", tuple(v.detach().reshape(-1).tolist()))
			if isinstance(v, np.ndarray):
				return ("a", tuple(v.reshape(-1).tolist()))
			if isinstance(v, dict):
				return tuple(sorted((str(k), freeze(x)) for k, x in v.items()))
			if isinstance(v, (list, tuple)):
				return tuple(freeze(x) for x in v)
			return v
		return (freeze(self.s), id(kernel), freeze(kernel.params_dict), tuple(kernel.operations))

	# ------------------------------------------------------------------ lazily materialised reference attributes
	@property
	def K(self):
		"""k(x,x) + Sigma^T Sigma (gauss_procc.py:163), recomputed on demand."""
		if not self.fitted:
			return np.array([1.0])              # gauss_procc.py:38
		xd = self._xd
		K = torch.empty((self.n, self.n), dtype=xd.dtype, device=xd.device)
		if self._Sigma is None:
			self.kernel_object._kernel_into(xd, xd, K, None, diag_add=float(self.s) ** 2)
		else:
			self.kernel_object._kernel_into(xd, xd, K, None)
			self._add_noise_gram(K, self._Sigma)
		return _lib.like_input(K, self.x)

	@property
	def Sigma(self):
		if self._Sigma is not None:
			return self._Sigma
		return self.s * torch.eye(self.n, dtype=torch.float64)

	def get_kernel(self):
		return self.K

	def norm(self):
		"""gauss_procc.py:179-184: sqrt(alpha^T k(x,x) alpha).  With (k + s^2 I) alpha = y this is
		sqrt(alpha^T y - s^2 alpha^T alpha): no n x n matrix is formed."""
		if not self.fitted:
			return None
		a = self._alpha.reshape(-1).contiguous()
		if self._Sigma is None:
			noise = float(self.s) ** 2 * float(_lib.trace_dot(u=a, v=a)[1].item())
		else:                                   # general noise matrix: alpha^T Sigma^T Sigma alpha = |Sigma alpha|^2
			Sd = _lib.to_device(self._Sigma, a.dtype).contiguous()
			v = torch.empty((1, Sd.shape[0]), dtype=a.dtype, device=a.device)
			_lib.gemm_nt(a.reshape(1, -1), Sd, v)
			v = v.reshape(-1)
			noise = float(_lib.trace_dot(u=v, v=v)[1].item())
		val = float(_lib.trace_dot(u=a, v=self._yd.reshape(-1).contiguous())[1].item()) - noise
		return _lib.like_input(torch.full((1, 1), math.sqrt(val) if val >= 0 else float("nan"), dtype=a.dtype), self.x)

	def beta(self, delta=1e-3, norm=1):
		"""gauss_procc.py:186-196: s * norm + sqrt(2 log(1/delta + log(det K / s^n))), K = k(x,x) + s^2 I.
		log det K comes from the factor (2 sum log L_ii), so nothing overflows at sizes where det K would."""
		L = self._L
		log_ratio = 2.0 * float(_lib.logdet_quad(L)[0].item()) - self.n * math.log(float(self.s))          # host scalars from here on
		arg = 1.0 / delta + log_ratio
		val = float(self.s) * norm + (math.sqrt(2.0 * math.log(arg)) if arg >= 1.0 else float("nan"))
		return _lib.like_input(torch.full((), val, dtype=L.dtype), self.x)

	# ------------------------------------------------------------------ prediction
	def execute(self, xtest):
		"""gauss_procc.py:198-209: (K* or None, K**)."""
		K_star = self.kernel(self._xd, _lib.to_device(xtest, self._xd.dtype)) if self.fitted else None
		if K_star is not None:
			K_star = _lib.like_input(K_star, xtest)
		K_star_star = self.kernel(xtest, xtest)
		return (K_star, K_star_star)

	def mean_std(self, xtest, full=False, reuse=False):
		"""gauss_procc.py:310-334: chunks of ``max_size`` test points against the resident factor."""
		m = xtest.size()[0]
		if _wants_grad(xtest):
			if full:
				raise ValueError("mean_std(full=True) has no input gradient: pass a test tensor without requires_grad")
			parts = [_PosteriorFn.apply(self, xtest[i0:i0 + self.max_size]) for i0 in range(0, m, self.max_size)]
			if len(parts) == 1:
				return parts[0]
			return torch.cat([p[0] for p in parts], dim=0), torch.cat([p[1] for p in parts], dim=0)
		if m < self.max_size or full:
			return self.mean_std_sub(xtest, full=full, reuse=reuse)
		dtype = self._xd.dtype if self.fitted else (xtest.dtype if xtest.dtype in (torch.float32, torch.float64) else torch.float64)
		mu = torch.zeros(size=(m, 1), dtype=dtype, device=xtest.device)
		std = torch.zeros(size=(m, 1), dtype=dtype, device=xtest.device)
		for i0 in range(0, m, self.max_size):
			mu[i0:i0 + self.max_size], std[i0:i0 + self.max_size] = self.mean_std_sub(xtest[i0:i0 + self.max_size, :], reuse=True)
		return mu, std

	mean_var = mean_std

	def mean_std_sub(self, xtest, full=False, reuse=False):
		"""gauss_procc.py:336-401 (squared loss)."""
		ko = self.kernel_object
		if not self.fitted:
			xt = _lib.to_device(xtest)
			if full:
				cov = torch.empty((xt.shape[0], xt.shape[0]), dtype=xt.dtype, device=xt.device)
				ko._kernel_into(xt, xt, cov)
				yvar = cov
			else:
				kd = torch.empty((xt.shape[0],), dtype=xt.dtype, device=xt.device)
				ko._diag_into(xt, kd)
				sd = torch.empty_like(kd)           # sqrt(diag K** - 0): the prediction epilogue with no data term
				_lib.predict_finish(sumsq=torch.zeros_like(kd), kdiag=kd, scale=0.0, sigma=sd)
				yvar = sd.reshape(-1, 1)
			zero = torch.zeros((xt.shape[0], 1), dtype=xt.dtype, device=xt.device)
			return (_lib.like_input(zero, xtest), _lib.like_input(yvar, xtest))

		xd = self._xd
		xt = _lib.to_device(xtest, xd.dtype)
		if not full:
			mu, sigma, _ = self._predict(xt)
			return (_lib.like_input(mu.reshape(-1, 1), xtest), _lib.like_input(sigma.reshape(-1, 1), xtest))
		m = xt.shape[0]
		X = self._solve_kstar(xt)[:m]
		mu = torch.empty((m,), dtype=xd.dtype, device=xd.device)
		_lib.predict(X, self._z, mu)
		cov = torch.empty((m, m), dtype=xd.dtype, device=xd.device)
		ko._kernel_into(xt, xt, cov)                                    # K**                      :343
		_lib.gemm_nt(X, X, cov, 1)                                      # K** - X X^T  :396-399
		return (_lib.like_input(mu.reshape(-1, 1), xtest), _lib.like_input(cov, xtest))

	def _solve_kstar(self, xt):
		"""X = K* L^-T (tile-padded: (mp, npad), zero rows past m and zero columns past n)."""
		xd = self._xd
		m, n0, n = xt.shape[0], self.n, self._L.shape[0]                # n: order of the (tile-padded) factor
		mp = _tile_pad(m)                                               # rows of K* padded to the tile as well (zero rows)
		X = torch.empty((mp, n), dtype=xd.dtype, device=xd.device)
		self.kernel_object._kernel_into(xd, xt, X[:m, :n0])             # K* = k(x, xtest): (M, N)   :346
		if n > n0:
			X[:, n0:].zero_()
		if mp > m:
			X[m:, :].zero_()
		_lib.trsm_right_lt(X, self._L, self._winv, self.nb, workspace=True)                 # X = K* L^-T
		return X

	def _predict(self, xt):
		"""mu, sigma (M,) and X = K* L^-T for device test points against the resident factor (gauss_procc.py:336-401, squared loss)."""
		xd = self._xd
		m = xt.shape[0]
		X = self._solve_kstar(xt)
		mu = torch.empty((m,), dtype=xd.dtype, device=xd.device)
		kd = torch.empty((m,), dtype=xd.dtype, device=xd.device)
		self.kernel_object._diag_into(xt, kd)                           # diag k(x*, x*)           :347
		sigma = torch.empty((m,), dtype=xd.dtype, device=xd.device)
		_lib.predict(X[:m], self._z, mu, sigma, kd, 1 if self.clamp_variance else 0)
		return mu, sigma, X

	# ------------------------------------------------------------------ input gradients (gauss_procc.py:420-459, :918-963)
	def _posterior(self, xtest):
		"""mu, sigma (M,) on the device and what their input gradient needs: (xt, X or None, sigma)."""
		if not self.fitted:
			xt = _lib.to_device(xtest)
			mu, sd = self.mean_std_sub(xt)
			sigma = sd.reshape(-1)
			return mu.reshape(-1), sigma, (xt, None, sigma)
		xt = _lib.to_device(xtest, self._xd.dtype)
		mu, sigma, X = self._predict(xt)
		return mu, sigma, (xt, X, sigma)

	def _weights_t(self, X):
		"""W^T = K* K^-1 = X L^-1 (in place over a copy of X): the variance gradient's coefficients, (mp, npad)."""
		Lr, winvr = self._factor.reversed()                              # built by the first variance gradient after a fit
		W = X.clone()
		_lib.trsm_right_ln(W, Lr, winvr, self.nb, workspace=True)
		return W

	def _posterior_grad(self, state, gmu, gstd):
		"""sum_t gmu_t grad mu(xt_t) + gstd_t grad sigma(xt_t), one row per test point: (M, d) on the device.
		grad sigma = (grad_x k(x, x) - 2 sum_i w_i grad_x k(x, x_i)) / (2 sigma), 0 where sigma is 0."""
		xt, X, sigma = state
		ko = self.kernel_object
		G = torch.zeros(xt.shape, dtype=xt.dtype, device=xt.device)
		u = None if gmu is None else _lib.to_device(gmu, xt.dtype).reshape(-1).contiguous()
		gs = None if gstd is None else _lib.to_device(gstd, xt.dtype).reshape(-1)
		if gs is not None and not bool((gs != 0).any()):
			gs = None
		if gs is not None:
			pos = sigma > 0
			safe = torch.where(pos, sigma, torch.ones_like(sigma))
			v = torch.where(pos, -gs / safe, torch.zeros_like(gs)).contiguous()
			self_coef = torch.where(pos, gs / (2.0 * safe), torch.zeros_like(gs))
		if X is not None and (u is not None or gs is not None):
			Wt = self._weights_t(X) if gs is not None else None
			ko._grad_into(self._xd, xt, G, alpha=self._alpha.reshape(-1).contiguous() if u is not None else None, u=u,
						  Wt=Wt, v=v if gs is not None else None)
		if gs is not None:
			ko._self_grad_into(xt, self_coef, G)
		return G

	def mean_std_grad(self, xtest):
		"""Batched input gradients of the posterior: (d mu, d std), each (M, d), where the inputs live."""
		mu, sigma, state = self._posterior(xtest.detach() if torch.is_tensor(xtest) else xtest)
		ones = torch.ones_like(sigma)
		dmu = self._posterior_grad(state, ones, None)
		dstd = self._posterior_grad(state, None, ones)
		return _lib.like_input(dmu, xtest), _lib.like_input(dstd, xtest)

	def mean_gradient_hessian(self, xtest, hessian=False):
		"""gauss_procc.py:444-459: the gradient (d,) of the posterior mean at the first row of xtest, and with ``hessian`` its
		Hessian (d, d) -- stpy_gram_grad with order 2 on alpha."""
		ko = self.kernel_object
		x1 = xtest[:1].detach() if torch.is_tensor(xtest) else xtest[:1]
		if not self.fitted:
			d = x1.shape[1]
			g, h = torch.zeros(d, dtype=torch.float64), torch.zeros((d, d), dtype=torch.float64)
			return [g, h] if hessian else g
		xt = _lib.to_device(x1, self._xd.dtype)
		d = xt.shape[1]
		G = torch.zeros((1, d), dtype=xt.dtype, device=xt.device)
		H = torch.zeros((1, d, d), dtype=xt.dtype, device=xt.device) if hessian else None
		ko._grad_into(self._xd, xt, G, alpha=self._alpha.reshape(-1).contiguous(), H=H)
		g = _lib.like_input(G[0], xtest)
		if not hessian:
			return g
		return [g, _lib.like_input(H[0], xtest)]

	def gradient_mean_var(self, point, hessian=False):
		"""gauss_procc.py:420-442: the gradient of the posterior mean at one point.  The reference's hessian=True branch calls
		KernelFunction.get_2_der / get_1_der, which do not exist there (it raises AttributeError)."""
		if hessian:
			raise NotImplementedError("gradient_mean_var(hessian=True): the reference calls kernel get_2_der / get_1_der, which do not "
									  "exist in stpy; use mean_gradient_hessian(x, hessian=True) for the mean's Hessian")
		return self.mean_gradient_hessian(point, hessian=False)

	def ucb_optimize(self, beta, multistart=25, lcb=False):
		"""
		gauss_procc.py:918-963: maximise mu + sqrt(beta) sigma (mu - sqrt(beta) sigma with ``lcb``) over ``self.bounds`` from
		``multistart`` uniform starts, drawn with the reference's np.random calls in its order.  All starts run as ONE L-BFGS-B
		problem over the stacked points (the objective is a sum of independent terms), so every step is one batched device
		evaluation of the values and their analytic gradients.  Returns (solution, value) of the best start.
		"""
		if self.bounds is None:
			raise ValueError("ucb_optimize needs box bounds: set GaussianProcess.bounds to a list of (low, high) per coordinate")
		starts = _draw_starts(multistart, self.d, self.bounds)
		sign = -1.0 if lcb else 1.0
		sb = float(np.sqrt(beta))
		dev = self._xd.device if self._xd is not None else _lib.device()
		dtype = self._xd.dtype if self._xd is not None else torch.float64

		def value(xt):
			mu, sigma, state = self._posterior(xt)
			return mu + sign * sb * sigma, state

		def evaluate(xt):
			val, state = value(xt)
			return val, self._posterior_grad(state, torch.ones_like(val), torch.full_like(val, sign * sb))

		sol, vals, _ = _multistart_maximize(evaluate, starts, self.bounds, dev, dtype, final=lambda xt: value(xt)[0])
		index = int(np.argmax(vals))
		return (torch.from_numpy(sol[index].copy()), torch.tensor(float(vals[index]), dtype=torch.float64))

	def mean(self, xtest):
		"""gauss_procc.py:403-418: K* alpha."""
		if _wants_grad(xtest):
			return _MeanFn.apply(self, xtest)
		return self._mean_value(xtest)

	def _mean_value(self, xtest):
		xd = self._xd
		xt = _lib.to_device(xtest, xd.dtype)
		m, n = xt.shape[0], self.n
		Ks = torch.empty((m, n), dtype=xd.dtype, device=xd.device)
		self.kernel_object._kernel_into(xd, xt, Ks)
		mu = torch.empty((m,), dtype=xd.dtype, device=xd.device)
		_lib.predict(Ks, self._alpha, mu)
		return _lib.like_input(mu.reshape(-1, 1), xtest)

	# ------------------------------------------------------------------ sampling
	def sample(self, xtest, size=1, jitter=10e-8):
		"""
		gauss_procc.py:461-482: f = mean + chol(Cov + 1e-9 I) r  (posterior, full covariance) or
		mu + chol(K** + jitter I) r (prior).  The standard-normal draws are taken exactly as in the
		reference -- torch.normal on the CPU generator, shape (nn, size) -- so a seeded reference run
		and a seeded run here see the same random_vector; the M x M Cholesky and the product run in
		stpy_potrf / stpy_gemm_nt.
		"""
		nn = list(xtest.size())[0]
		if self.fitted == True:
			(ymean, cov) = self.mean_std(xtest, full=True)
			eps = 10e-10
		else:
			(_, cov) = self.execute(xtest)
			ymean = self.mu
			eps = jitter
		cov = _lib.to_device(cov)
		C = torch.empty_like(cov)
		_lib.combine(C, cov, _lib.OUT_SET, eps)                                        # C = cov + eps I
		_, info = _lib.potrf(C, self.nb)
		self._check_info(info, "sample: posterior covariance + jitter is not positive definite (leading minor %d)")
		_lib.tril(C)                        # the strict upper triangle of an in-place factor is scratch
		random_vector = torch.normal(mean=torch.zeros(nn, size, dtype=torch.float64), std=1.)
		rt = random_vector.T.contiguous().to(device=C.device, dtype=C.dtype)          # (size, nn): the NT operand
		# f = ymean + L r: the accumulating product on a result that starts as the mean in every column
		f = torch.empty((nn, size), dtype=C.dtype, device=C.device)
		if torch.is_tensor(ymean):
			f.copy_(_lib.to_device(ymean, C.dtype).reshape(nn, 1).expand(nn, size))
		else:
			f.fill_(float(ymean))
		_lib.gemm_nt(C, rt, f, 2)
		return _lib.like_input(f, xtest)

	def sample_and_max(self, xtest, size=1):
		"""gauss_procc.py:484-494."""
		f = self.sample(xtest, size=size)
		self.temp = f
		val, index = torch.max(f, dim=0)
		return (xtest[index, :], val)

	# ------------------------------------------------------------------ evidence
	def log_marginal(self, kernel, X, weight):
		"""
		gauss_procc.py:497-504 -> :631-638 (== estimator.py:32-40):
		    1/2 y^T (K_theta + s^2 I)^-1 y + 1/2 * weight * log det(K_theta + s^2 I),   shape (1, 1).
		Negative log evidence without the n/2 log(2 pi) constant.  ``X`` holds per-item parameter
		overrides in the kwargs protocol of kernels.py:138-157.  With X empty and ``kernel`` the
		fitted kernel object, the resident factor is reused.

		If a lengthscale tensor in ``X`` ('gamma' / 'ard_gamma'), the map of a full-covariance item ('cov') or the noise ``self.s`` requires grad --
		the way Estimator.optimize_params_general drives this method (estimator.py:156-190) -- the
		result carries an autograd node whose backward is the analytic evidence gradient
		1/2 tr((w K^-1 - alpha alpha^T) dK/dtheta) evaluated on the device (stpy_potri,
		stpy_lml_weight, stpy_gemm_nt).
		"""
		params = self._grad_params(X, _GRAD_NAMES)
		if params:
			return _LogMarginalFn.apply(self, kernel, X, weight, *[t for (_, _, t) in params])
		return self._log_marginal_value(kernel, X, weight)[0]

	def _ensure_device_data(self, caller):
		"""Data handed over by ``load_data`` goes to the device at its first use."""
		if self._xd is None:
			if self.x is None:
				raise AttributeError("%s needs data: call fit_gp or load_data first" % caller)
			self._xd = _lib.to_device(self.x)
			self._yd = _lib.to_device(self.y, self._xd.dtype).reshape(-1, 1)
			self.n = self._xd.shape[0]

	def _log_marginal_value(self, kernel, X, weight):
		self._ensure_device_data("log_marginal")
		F = self._factor
		if not (self.fitted and F is not None and (not X) and (kernel is self.kernel_object) and self._Sigma is None
				and F.key == self._hyper_key(kernel)):
			F, info = self._factorize(kernel, self._xd, X)                  # a factor of this call alone: the resident one stays
			self._check_info(info)
			F.z = _lib.trsv(F.L, F.winv, self._yd)
		L = F.L
		out2 = _lib.logdet_quad(L, F.z)
		w = _weight(weight)
		logdiag, quad = out2.tolist()                                                   # sum log L_ii, z^T z: host scalars
		val = torch.full((1, 1), 0.5 * quad + 0.5 * w * 2.0 * logdiag, dtype=L.dtype, device=L.device)
		return _lib.like_input(val, self.x), F

	def _log_marginal_grads(self, kernel, X, weight, state, params):
		"""
		d/dtheta of the value above for every entry of ``params`` (same order), as tensors shaped like the parameters.

		G = w K^-1 - alpha alpha^T (stpy_potri).  The kernel is a chain of items combined by + and *
		(kernels.py:146-157), every item a sum of terms kappa phi(scaled distance).  For a lengthscale l_m of
		a term t of item i:   dK/dl_m = M_i o kappa F_t u_m^2 / l_m,   u_m the scaled coordinate difference, F_t the
		family's derivative factor, and M_i = dK/dK_i the elementwise product of everything item i is multiplied
		with (the value accumulated before it when its own operation is *, and every later item joined by *).
		So H = G o kappa F_t (stpy_lml_weight) o M_i (stpy_gram with the multiply combine), and
		sum_ij H_ij u_m^2 = 2 [ sum_i xs_im^2 h_i - xs_m^T H xs_m ] with h = H 1 -- one stpy_gemm_nt of H
		against [Xs | 1].
		"""
		L, winv, z = state.L, state.winv, state.z
		npad = L.shape[0]                               # tile-padded order of the factor (see _factorize)
		items = kernel._chain(X)
		w = _weight(weight)
		xd = self._xd
		n = xd.shape[0]
		alpha = _lib.trsv(L, winv, z, trans=1)[:n]
		# inverse of the bordered matrix = [[K^-1, 0], [0, I]]: everything below works on the leading n x n views (the potri
		# workspace is kept as the scratch H of several kernel terms)
		work_p = torch.empty((npad, npad), dtype=L.dtype, device=L.device)
		Kinv = _lib.potri(L, winv, n, work=work_p)
		work = work_p[:n, :n]
		td = _lib.trace_dot(Kinv, alpha, alpha)                                          # tr(K^-1), alpha^T alpha: fixed-order reduction

		wanted = [(key, name, t) for (key, name, t) in params if key != "likelihood"]
		single = len(items) == 1 and len(items[0]['terms']) == 1
		acc = {(key, name): torch.zeros(t.numel(), dtype=L.dtype, device=L.device) for (key, name, t) in wanted}
		tmp = None
		for i, it in enumerate(items):
			mine = [(key, name) for (key, name, _) in wanted if key == str(i)]
			if not mine:
				continue
			for term in it['terms']:
				if term['pname'] is None or (str(i), term['pname']) not in acc:
					continue
				premap = term['premap']
				group = term['group']
				cols, inv_ls = kernel._term_operands(term, xd, xd.dtype, xd.device)
				if premap is not None:
					# full-covariance item (kernels.py:464-549): the points enter as z = x[:, group] cov with unit lengthscales; the
					# parameter is the map itself.  d/dcov[a][m] = -1/2 sum_ij H_ij (z_i - z_j)_m (x_i - x_j)_a  (stpy_lml_grad_cov_reduce)
					kx = kernel._premap(xd, group, premap)                       # (n, p): what the weight / product kernels see as "the points"
					kcols, kd = None, kx.shape[1]
				else:
					kx, kcols, kd = xd, cols, len(group)
				# H <- (w K^-1 - alpha alpha^T) o kappa F_t: in place over K^-1 when this is the only term, otherwise written
				# to `work` with K^-1 only read (no N x N copy)
				H = Kinv if single else work
				_lib.lml_weight(term['kind'], kx, inv_ls, term['kappa'], w, alpha, Kinv, H, cols=kcols)
				# ... o M_i (a single-term factor multiplies straight into H; the scratch of the others is kept for the next term)
				tmp = kernel._mul_factors_into(items, i, xd, xd, H, tmp)
				# [Xs | 1]^T (dg + 1, n): scaled coordinates as the NT operand, then P = H [Xs | 1] and the per-coordinate sums (for the
				# lengthscale sums the coordinates are taken relative to the first point: the sums do not see the translation, their
				# rounding does; the full-covariance reduction works on the points as they are)
				dg = kd
				XT = _lib.scaled_points_t(kx, inv_ls, kcols, centre=premap is None)
				P = torch.empty((n, dg + 1), dtype=xd.dtype, device=xd.device)
				_lib.gemm_nt(H, XT, P)
				a_ = acc[(str(i), term['pname'])]
				if premap is not None:
					if a_.numel() != len(group) * dg:
						raise ValueError("evidence gradient: 'cov' has %d entries, the item maps %d columns to %d" % (a_.numel(), len(group), dg))
					_lib.lml_grad_cov_reduce(xd, kx, P, a_, cols)
					continue
				_lib.lml_grad_reduce(xd, inv_ls, P, kernel._term_param_slots(term, xd.device), a_, cols, centred=True)
		del work, work_p
		for key, name, t in wanted:
			if (key, name) not in acc or int(key) >= len(items) or not any(tm['pname'] == name for tm in items[int(key)]['terms']):
				raise NotImplementedError("evidence gradient: kernel item %s has no '%s' lengthscale on the device path" % (key, name))
		grads = []
		for (key, name, t) in params:
			if key == "likelihood":      # noise std: dK/ds = 2 s I  =>  s tr(w K^-1 - alpha alpha^T), host scalars
				sval = float(t.detach().reshape(-1)[0].item())
				trK, aa = td.tolist()
				g = torch.full(t.shape if t.dim() > 0 else (), sval * (w * trK - aa), dtype=L.dtype)
			else:
				g = acc[(key, name)].reshape(t.shape if t.dim() > 0 else ())
			grads.append(g.to(device=t.device, dtype=t.dtype))
		return grads

	# ------------------------------------------------------------------ evidence of several candidates in one launch
	# Largest n at which log_marginal_batch takes the batched device kernel (never above the library's own cap, stpy_lml_batch_max_n):
	# the largest measured n at which eight batched evaluations beat eight serial ones by more than the serial loop's run-to-run
	# spread (tools/lml_batch_bench.py; DESIGN.md "Batched evidence for restarts"): 3.3 against 6.1 ms at n = 512, the cap itself.
	lml_batch_max_n = 512

	def _lml_batch_plan(self, kernel, Xs):
		"""What stpy_lml_batch needs for the candidates ``Xs``, or None when the batch kernel does not cover them: a single-GPU
		GaussianProcess on fp64 data of at most ``lml_batch_max_n`` points without an explicit Sigma, and a kernel that resolves to ONE
		item with ONE term of the SE / Matern 1/2, 3/2, 5/2 families without a pre-map -- the same family, kappa and columns for every
		candidate.  Returns (term of the first candidate, inverse lengthscales (B, d), parameter shape)."""
		if type(self) is not GaussianProcess or self._Sigma is not None or not hasattr(kernel, "_resolve") or len(Xs) == 0:
			return None
		xd = self._xd
		if xd.dtype != torch.float64 or xd.shape[0] > min(int(self.lml_batch_max_n), _lib.lml_batch_max_n()) or xd.shape[0] == 0:
			return None
		first, rows, shape = None, [], None
		for X in Xs:
			items = kernel._resolve({k: dict(v) for k, v in X.items()} if X else {})
			if len(items) != 1 or len(items[0]['terms']) != 1:
				return None
			t = items[0]['terms'][0]
			if t['premap'] is not None or t['pname'] is None or t['kind'] not in (_lib.K_SE, _lib.K_MATERN12, _lib.K_MATERN32, _lib.K_MATERN52):
				return None
			if first is None:
				first = t
			elif (t['kind'], t['kappa'], t['group'], t['pidx'], t['pname']) != (first['kind'], first['kappa'], first['group'], first['pidx'], first['pname']):
				return None
			rows.append(t['inv_ls'])
			v = X.get('0', {}).get(t['pname']) if X else None
			sh = tuple(torch.as_tensor(v).shape) if v is not None else (max(t['pidx']) + 1,)
			if shape is None:
				shape = sh
			elif sh != shape:
				return None
		if int(np.prod(shape)) < max(first['pidx']) + 1:
			return None
		return first, np.asarray(rows, dtype=np.float64), shape

	def log_marginal_batch(self, kernel, Xs, weight, s=None):
		"""
		``log_marginal`` and its gradient for B candidates at once -- the restarts of a hyper-parameter search.  ``Xs``: a list of
		override dictionaries in the protocol ``log_marginal`` takes; ``s``: optional noise stds, one per candidate (None: ``self.s``
		for all, and no noise gradient).  Returns (values (B,) placed like the data, grads): ``grads[b]`` = {item key: {parameter
		name: tensor shaped like the parameter}}, plus {'likelihood': {'sigma': ...}} when ``s`` is given.  A candidate whose matrix is
		not positive definite gets +inf and zero gradients, no exception: one bad candidate does not void the rest.

		Where ``_lml_batch_plan`` allows it, all candidates are ONE launch of stpy_lml_batch (one workgroup per candidate; inverse
		lengthscales, noise and parameter slots go up in one copy, values, gradients and status come back in one); otherwise they
		run one after another through ``log_marginal`` (``Estimator.log_marginal_batch``).  ``self.lml_batch_path`` says which:
		"device" or "serial".
		"""
		self._ensure_device_data("log_marginal_batch")
		plan = self._lml_batch_plan(kernel, Xs)
		if plan is None:
			return super().log_marginal_batch(kernel, Xs, weight, s)
		term, inv_ls, shape = plan
		xd = self._xd
		B, d = inv_ls.shape
		n_params = int(np.prod(shape))
		w = _weight(weight)
		noise = np.full(B, float(self.s)) if s is None else np.asarray([float(v) for v in s], dtype=np.float64)
		if noise.shape[0] != B:
			raise ValueError("log_marginal_batch: %d noise levels for %d candidates" % (noise.shape[0], B))
		# one upload: [inverse lengthscales | noise | parameter slots (int32, two to a double)]
		host = np.zeros(B * d + B + (d + 1) // 2, dtype=np.float64)
		host[:B * d] = inv_ls.reshape(-1)
		host[B * d:B * d + B] = noise
		host[B * d + B:].view(np.int32)[:d] = np.asarray(term['pidx'], dtype=np.int32)
		dev = torch.from_numpy(host).to(xd.device)
		cols, _ = kernel._term_operands(term, xd, xd.dtype, xd.device)
		_, _, _, packed = _lib.lml_batch(term['kind'], xd, self._yd.reshape(-1), dev[:B * d].view(B, d), dev[B * d:B * d + B],
										 dev[B * d + B:].view(torch.int32)[:d], n_params, term['kappa'], w, cols=cols)
		out = packed.cpu().numpy()          # the one read-back (waits for the launch)
		ldg = n_params + 1
		values = out[:B * 8].view(np.float64).copy()
		grad = out[B * 8:B * (ldg + 1) * 8].view(np.float64).reshape(B, ldg)
		info = out[B * (ldg + 1) * 8:].view(np.int32)
		self.lml_batch_path = "device"
		self.lml_batch_info = info.copy()
		grads = []
		for b in range(B):
			g = {'0': {term['pname']: torch.from_numpy(grad[b, :n_params].copy()).reshape(shape)}}
			if s is not None:
				g['likelihood'] = {'sigma': torch.from_numpy(grad[b, n_params:ldg].copy())}
			grads.append(g)
		values = torch.from_numpy(values)
		return (values.to(self.x.device) if torch.is_tensor(self.x) and self.x.is_cuda else values), grads

	# ------------------------------------------------------------------ hyper-parameter search (caller of the hot path)
	def optimize_params(self, type='bandwidth', restarts=10, regularizer=None,
						maxiter=1000, mingradnorm=1e-4, verbose=False, optimizer="pymanopt", scale=1., weight=1., save=False,
						save_name='model.np', init_func=None, bounds=None, parallel=False, cores=None):
		"""
		gauss_procc.py:640-702 for ``type`` in {"bandwidth", "bandwidth+noise"}: builds the ``params`` dictionary -- every
		kernel item's 'gamma' / 'ard_gamma' on a Euclidean factor, optionally the noise std under the key 'likelihood' -- and
		hands it to ``Estimator.optimize_params_general`` (stpy_amd/estimator.py), which minimises ``log_marginal`` over
		``restarts`` starting points, writes the best one back into ``kernel_object.params_dict`` / ``self.s`` and refits.
		Objective and gradient are the device evidence and its analytic gradient (every evaluation is a full Gram +
		Cholesky [+ inverse]); with ``parallel=True`` the restarts are evaluated together, one ``log_marginal_batch`` call -- one
		stpy_lml_batch launch where the kernel is covered -- per step (``cores`` is accepted and unused).  The rotation / group / covariance searches of the reference (Stiefel and PSD manifolds,
		discrete group enumeration) are outside the hot path.
		"""
		if regularizer is not None:
			if regularizer[0] == "spectral_norm":          # gauss_procc.py:645-653
				regularizer_func = lambda S: regularizer[1] * torch.norm(1 / S.reshape(1, -1), p='nuc')
			elif regularizer[0] == 'lasso':
				regularizer_func = lambda S: regularizer[1] * torch.norm(1 / S, p=1)
			else:
				regularizer_func = None
		else:
			regularizer_func = None
		if type not in ("bandwidth", "bandwidth+noise"):
			if type in ("rots", "groups", "covariance"):
				raise NotImplementedError("optimize_params(type='%s') is outside the stpy_amd hot path" % type)
			raise AttributeError("This quick-optimization is not implemented.")          # gauss_procc.py:698
		params = self._bandwidth_params(type, init_func, bounds)
		return self.optimize_params_general(params=params, restarts=restarts, optimizer=optimizer, regularizer_func=regularizer_func,
											maxiter=maxiter, mingradnorm=mingradnorm, verbose=verbose, scale=scale, weight=weight,
											save=save, save_name=save_name, parallel=parallel, cores=cores)

	def load_data(self, d):
		"""estimator.py:28-30."""
		self.x = d[0]
		self.y = d[1]
		self._xd = self._yd = None
		self.n = self.x.shape[0]
