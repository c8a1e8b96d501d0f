"""
Drop-in for ``stpy.continuous_processes.nystrom_fea.NystromFeatures`` (reference: nystrom_fea.py:11-35 ctor / description, :46-50 uniform
subsampling, :106-207 fit_gp, :209-259 mean_std / outer_kernel / sample_theta / sample), plus a landmark choice the reference does not
have: greedy pivoted partial Cholesky of the kernel matrix (``approx="pivoted"``, ``stpy_pchol``, csrc/pchol.hip).

With landmarks P the reference maps q to D^-1/2 V^T k(x_P, q) from the eigendecomposition K_PP = V D V^T (:188-197).  Here
    phi(q) = L^-1 k(x_P, q),      L L^T = K_PP + jitter kappa I          (stpy_gram, stpy_potrf, stpy_trsm_right_lt)
which is the same map up to a rotation of feature space: both give the approximate kernel k(q, x_P) K_PP^-1 k(x_P, q'), so feature Gram
matrices, ridge predictions and posterior draws' distribution are those of the reference; no eigendecomposition is needed.  The map
acts row by row, so ``KernelizedFeatures`` can stream it over row slabs, and that is what ``mean_std`` / ``sample_theta`` / ``sample``
delegate to (primal ridge with lam = 1: nystrom_fea.py:209-259 without ``torch.solve``).

Landmarks by ``approx``:
  "uniform"   np.random.choice(N, ms) with replacement, drawn where the reference draws it (or ``indices``); repeated indices are dropped
              (first occurrences kept).  The reference zeroes the feature of a zero eigenvalue (:192-194); to match, the map keeps ``ms``
              columns and those beyond the distinct landmarks are zero.
  "nothing"   the first ms rows and M = I (:138-141): phi(q) = k(x_P, q), no factor.
  "pivoted"   the pivots of ``stpy_pchol`` with tolerance ``tol``; a rank below ms zero-pads in the same way.  ``trace_error`` is the sum of
              the residual diagonal, trace(K - F F^T): the trace-norm error of the rank-r approximation, a 0-d device tensor (reading it
              is the caller's synchronisation).  Single-term SE / Matern / ARD kernel objects only.
  "leverage", "online_leverage", "svd", "positive_svd", "cover" are bound by a full GP fit per point, an N x N eigendecomposition, NMF or
  a matrix square root, and raise NotImplementedError.
Input gradients are out of scope: ``_operands`` keeps the base class's NotImplementedError, so autograd through ``KernelizedFeatures`` on
this embedding raises clearly.
"""
import numpy as np
import torch

from .. import _lib
from ..embeddings.embedding import Embedding

_APPROX_OUT_OF_SCOPE = {
	"leverage": "leverage-score sampling fits an exact GP on all N points first (nystrom_fea.py:52-76)",
	"online_leverage": "sequential leverage scores refit a GP for every candidate point (nystrom_fea.py:78-104)",
	"svd": "the top eigenvectors of the N x N kernel matrix are eigendecomposition-bound (nystrom_fea.py:116-137)",
	"positive_svd": "non-negative matrix factorisation of GP samples (sklearn NMF, nystrom_fea.py:143-176)",
	"cover": "the matrix square root of the N x N kernel matrix (scipy sqrtm, nystrom_fea.py:178-183)",
}
_STATIONARY = (_lib.K_SE, _lib.K_MATERN12, _lib.K_MATERN32, _lib.K_MATERN52)


def _stationary_term(kernel_object):
	"""The one launch description of a single-term SE / Matern / ARD kernel object; NotImplementedError for anything else.  Host only."""
	items = kernel_object._chain()
	if len(items) != 1 or len(items[0]['terms']) != 1:
		raise NotImplementedError("pivoted Cholesky needs a single-term kernel (one SE / Matern / ARD item); this one has %d items, the first "
								  "of %d terms" % (len(items), len(items[0]['terms']) if items else 0))
	t = items[0]['terms'][0]
	if t['premap'] is not None or t['kind'] not in _STATIONARY:
		raise NotImplementedError("pivoted Cholesky supports SE / Matern / ARD kernels; got the %s kernel" % kernel_object._term_name(t))
	return t


_OVERRIDE_KEYS = ("gamma", "ard_gamma", "kappa", "group", "offset", "nu")


def _check_term_overrides(who, owner, own_kernel, kernel, X, supported="'gamma' / 'ard_gamma'"):
	"""Host refusals of an evidence that covers ONE stationary term and differentiates its lengthscales and the noise only: returns (X or {},
	the one term ``kernel`` resolves to under the overrides ``X``).  ``who`` ("Class.method") and ``owner`` (what has the one item) word the messages."""
	X = {} if X is None else X
	if kernel is not own_kernel:
		_stationary_term(kernel)
	for key, item in X.items():
		if str(key) != "0" or not isinstance(item, dict):
			raise NotImplementedError("%s: overrides for kernel item %r; %s has ONE item, '0'" % (who, key, owner))
		for name, v in item.items():
			if name not in _OVERRIDE_KEYS:
				raise NotImplementedError("%s: override %r is not a lengthscale of a single stationary term (supported: %s)" % (who, name, supported))
			if name not in ("gamma", "ard_gamma") and torch.is_tensor(v) and v.requires_grad:
				raise NotImplementedError("%s: no gradient with respect to %r (lengthscales and the noise only)" % (who, name))
	items = kernel._chain(X if X else None)
	if len(items) != 1 or len(items[0]['terms']) != 1:
		raise NotImplementedError("%s: the overrides resolve to %d items; ONE stationary term is supported" % (who, len(items)))
	return X, items[0]['terms'][0]


def _pchol_device(kernel_object, xd, m, tol):
	t = _stationary_term(kernel_object)
	cols, inv_ls = kernel_object._term_operands(t, xd, xd.dtype, xd.device)
	return _lib.pchol(t['kind'], xd, inv_ls, int(m), cols=cols, kappa=t['kappa'], tol=float(tol))


def pivoted_cholesky(kernel_object, x, m, tol=0.):
	"""Greedy pivoted partial Cholesky of kernel_object.kernel(x, x) in at most m steps, never forming the matrix (stpy_pchol).
	Returns (piv (r,) int32, F (n, r) with F F^T ~ K, dres (n,) = diag(K - F F^T), rank r), tensors where x lives."""
	_stationary_term(kernel_object)
	xd = _lib.to_device(x)
	piv, Ft, dres, rank = _pchol_device(kernel_object, xd, m, tol)
	r = int(rank.item())
	return _lib.like_input(piv[:r], x), _lib.like_input(Ft[:r].t(), x), _lib.like_input(dres, x), r


class NystromFeatures(Embedding):
	"""nystrom_fea.py:11-259."""

	def __init__(self, kernel_object, m=100, approx="uniform", s=1., samples=100, *, tol=0., jitter=0.):
		self.kernel_object, self.kernel = kernel_object, kernel_object.kernel
		self.m, self.ms = m, int(torch.as_tensor(m).sum())          # (m may be a tensor of per-group counts, as for the other embeddings)
		self.approx, self.s, self.samples = approx, s, samples
		self.fit = False
		self.tol = tol
		self.jitter = jitter
		self.x = self.y = None
		self.C = []
		self.trace_error = None
		self._xP = self._L = self._winv = self._kf = None
		self._check()

	def _check(self):
		"""Everything that can be refused is refused here, on the host: before a fit touches the device."""
		if self.approx in _APPROX_OUT_OF_SCOPE:
			raise NotImplementedError("NystromFeatures(approx='%s') is outside the stpy_amd hot path: %s" % (self.approx, _APPROX_OUT_OF_SCOPE[self.approx]))
		if self.approx not in ("uniform", "nothing", "pivoted"):
			raise NotImplementedError("NystromFeatures: unknown approx '%s' (uniform, nothing, pivoted)" % self.approx)
		if self.approx == "pivoted":
			_stationary_term(self.kernel_object)
		if not (float(self.tol) >= 0.0 and float(self.jitter) >= 0.0):
			raise ValueError("NystromFeatures: tol and jitter must not be negative")

	def description(self):
		return "Nystrom features, %d landmarks chosen by '%s'" % (self.ms, self.approx)

	def get_m(self):
		return int(self.ms)

	# ------------------------------------------------------------------ fit
	def fit_gp(self, x, y, eps=1e-14, indices=None):
		"""nystrom_fea.py:106-207: picks the landmarks and keeps (L, winv, x_P) on the device."""
		self._check()
		self.x, self.y = x, y
		self.d = x.size()[1]
		self.N = x.size()[0]
		assert (self.ms <= self.N)
		self.fit = False
		self._kf = None
		self.trace_error = None
		if self.approx == "uniform":
			# the reference's draw (nystrom_fea.py:48): with replacement, from the global numpy generator, the first thing a fit draws
			self.C = np.random.choice(self.N, self.ms) if indices is None else np.asarray(indices).reshape(-1)
			seen, landmarks = set(), []
			for c in self.C:
				c = int(c)
				if not 0 <= c < self.N:
					raise IndexError("NystromFeatures: landmark index %d outside [0, %d)" % (c, self.N))
				if c not in seen:
					seen.add(c)
					landmarks.append(c)
			if len(landmarks) > self.ms:
				raise ValueError("NystromFeatures: %d landmarks for %d features" % (len(landmarks), self.ms))
		xd = _lib.to_device(x)
		if self.approx == "nothing":
			self.C = np.arange(self.ms)
			self._xP = xd[:self.ms].contiguous()
			self._L = self._winv = None
			self.fit = True
			return None
		if self.approx == "pivoted":
			piv, _, dres, rank = _pchol_device(self.kernel_object, xd, self.ms, self.tol)
			self.trace_error = _lib.trace_dot(u=dres, v=torch.ones_like(dres))[1]          # sum of the residual diagonal, fixed order; unread
			r = int(rank.item())
			if r < 1:
				raise torch.linalg.LinAlgError("NystromFeatures: the pivoted Cholesky stopped at rank 0 (kappa <= 0, or tol >= 1)")
			idx = piv[:r].long()
			self.C = piv[:r].cpu().numpy()
		else:
			idx = torch.as_tensor(landmarks, dtype=torch.long, device=xd.device)
		self._xP = xd.index_select(0, idx).contiguous()
		r = self._xP.shape[0]
		Kpp = torch.empty((r, r), dtype=xd.dtype, device=xd.device)
		diag_add = 0.0
		if float(self.jitter) != 0.0:
			kap = torch.empty((1,), dtype=xd.dtype, device=xd.device)
			self.kernel_object._diag_into(self._xP[:1], kap)
			diag_add = float(self.jitter) * float(kap.item())
		self.kernel_object._kernel_into(self._xP, self._xP, Kpp, None, diag_add=diag_add, lower_only=True)
		winv, info = _lib.potrf(Kpp)
		bad = int(info.item())
		if bad != 0:
			raise torch.linalg.LinAlgError("NystromFeatures: the landmark kernel matrix K_PP + jitter kappa I (jitter = %g) is not positive definite "
										   "(leading minor %d of %d); raise `jitter`, or pick landmarks with approx='pivoted' and a tol > 0" % (float(self.jitter), bad, r))
		self._L, self._winv = Kpp, winv
		self.fit = True
		return None

	# ------------------------------------------------------------------ the map
	def embed(self, q):
		"""(n_q, ms): rows L^-1 k(x_P, q_i), zero beyond the landmark count."""
		if not self.fit:
			raise AssertionError("First fit")
		qd = _lib.to_device(q, self._xP.dtype)
		r = self._xP.shape[0]
		B = torch.empty((qd.shape[0], self.get_m()), dtype=qd.dtype, device=qd.device)
		if r < B.shape[1]:
			B[:, r:].zero_()
		if qd.shape[0] == 0:
			return _lib.like_input(B, q)
		Br = B[:, :r]
		self.kernel_object._kernel_into(self._xP, qd, Br)                  # k(x_P, q): (n_q, r), rows = right-hand sides
		if self._L is not None:
			_lib.trsm_right_lt(Br, self._L, self._winv)
		return _lib.like_input(B, q)

	# ------------------------------------------------------------------ the estimator on the features (nystrom_fea.py:209-259)
	def _estimator(self):
		if not self.fit:
			raise AssertionError("First fit")
		if self._kf is None:
			from .kernelized_features import KernelizedFeatures
			kf = KernelizedFeatures(embedding=self, m=self.get_m(), s=self.s, lam=1.)
			kf.fit_gp(self.x, self.y)
			self._kf = kf
		return self._kf

	def mean_std(self, xtest):
		return self._estimator().mean_std(xtest)

	def sample_theta(self, size=1):
		return self._estimator().sample_theta(size=size)

	def sample(self, xtest, size=1):
		return self._estimator().sample(xtest, size=size)

	def outer_kernel(self):
		"""nystrom_fea.py:223-232: Phi Phi^T + s^2 I, N x N -- small N only."""
		Phi = _lib.to_device(self.embed(_lib.to_device(self.x)))
		K = torch.empty((Phi.shape[0], Phi.shape[0]), dtype=Phi.dtype, device=Phi.device)
		_lib.gemm_nt(Phi, Phi, K)
		_lib.combine(K, K, _lib.OUT_SET, float(self.s) ** 2)
		return _lib.like_input(K, self.x)
