"""
Exact GP regression without the N x N matrix: ``IterativeGaussianProcess`` solves (K + s^2 I) alpha = y by preconditioned conjugate
gradients on an operator that is generated from the points on the fly (stpy_kmv / stpy_pcg, csrc/kmv.hip).  The reference has no such
route (gauss_procc.py factors K); the interface is that of ``GaussianProcess`` for the part that a matrix-free solve can serve.

Memory is O(N (r + t)) -- the rank-r preconditioner and the CG state for t right-hand sides -- instead of 8 N^2 bytes, so one device
holds problems whose factor it cannot.  The price: every solve is iterative, and the posterior variance needs one solve per test point.

  fit_gp      stpy_pchol on the training points (rank r <= min(precond_rank, N), early stop by precond_tol); C = s^2 I + F^T F (stpy_syrk),
              C = L L^T (stpy_potrf), G = F L^-T (stpy_trsm_right_lt): M^-1 = I - G G^T is s^2 times the Woodbury inverse of s^2 I + F F^T.
              Then stpy_pcg in blocks of ``check_every`` iterations; the host reads the residuals between blocks.
  mean        ONE rectangular stpy_kmv (a = xtest, b = x, Vt = alpha^T): K* is never stored.  The cheap path.
  mean_std    the mean as above; the variance by BLOCK SOLVES, one stpy_pcg solve per ``rhs_block`` test points, each as expensive as the fit
              (t columns share every kernel evaluation, so a block costs about one fit, not rhs_block fits).  sigma = sqrt(kdiag - <k*, A^-1 k*>).

Out of scope, each for its own reason (all raise NotImplementedError before the device is touched):
  log_marginal / optimize_params   the log-determinant of a matrix that is never formed needs stochastic Lanczos quadrature, an estimator with
                                   its own variance and probe count: a different contract from the exact evidence the other classes return;
  sample                           a posterior draw needs a square root of the N x N posterior covariance (Lanczos or pathwise conditioning);
  input gradients                  (a test tensor with requires_grad) the gradient of the variance needs K*' A^-1 k*, more solves per point;
  composite kernels                the operator is evaluated inside the kernel for ONE stationary term (SE / Matern / ARD), the terms the pivoted
                                   Cholesky preconditioner covers as well;
  Sigma                            a general noise matrix is a second dense N x N operand;
  multi-GPU                        the row split of the operator needs its own reduction of the CG scalars across ranks.
"""
import numpy as np
import torch

from .. import _lib
from ..estimator import Estimator
from ..kernels import KernelFunction
from .nystrom_fea import _stationary_term

_OUT_OF_SCOPE = {
	"log_marginal": "the log-determinant of a matrix that is never formed needs stochastic Lanczos quadrature (a randomised estimate, not the exact evidence)",
	"optimize_params": "it minimises log_marginal, whose log-determinant needs stochastic Lanczos quadrature here",
	"sample": "a posterior draw needs a square root of the N x N posterior covariance, which this class never forms",
}


class IterativeGaussianProcess(Estimator):

	def __init__(self, gamma=1, s=0.001, kappa=1., kernel_name="squared_exponential", d=1, kernel=None,
				 precond_rank=256, precond_tol=0., tol=None, maxiter=1000, check_every=10, rhs_block=64, nu=1.5):
		self.s = s
		self.d = d
		self.x = self.y = None
		self.n = 0
		self.fitted = False
		if kernel is not None:
			self.kernel_object = kernel
			self.d = kernel.d
		else:
			self.kernel_object = KernelFunction(kernel_name=kernel_name, gamma=gamma, nu=nu, kappa=kappa, d=d)
		self.kernel = self.kernel_object.kernel
		self.precond_rank, self.precond_tol = int(precond_rank), float(precond_tol)
		self.tol, self.maxiter, self.check_every, self.rhs_block = tol, int(maxiter), int(check_every), int(rhs_block)
		self.trace_error = None
		self.cg_info = {"iterations": 0, "relres": 0.0, "rank": 0, "kmv_launches": 0}
		self._xd = self._alpha = self._Gt = self._Gn = None
		self._kmv_launches = 0
		self._check()

	def _check(self):
		"""Everything that can be refused is refused here, on the host."""
		_stationary_term(self.kernel_object)
		if self.precond_rank < 0 or not self.precond_tol >= 0.0:
			raise ValueError("IterativeGaussianProcess: precond_rank and precond_tol must not be negative")
		if self.maxiter < 1 or self.check_every < 1 or self.rhs_block < 1:
			raise ValueError("IterativeGaussianProcess: maxiter, check_every and rhs_block must be positive")
		if self.tol is not None and not float(self.tol) > 0.0:
			raise ValueError("IterativeGaussianProcess: tol must be positive")

	def description(self):
		return self.kernel_object.description() + "\nlambda=" + str(self.s) + "\nmatrix-free (preconditioned CG, rank <= %d)" % self.precond_rank

	def _tol(self, dtype):
		return float(self.tol) if self.tol is not None else (1e-8 if dtype == torch.float64 else 1e-4)

	# ------------------------------------------------------------------ refusals
	def log_marginal(self, *args, **kwargs):
		raise NotImplementedError("IterativeGaussianProcess.log_marginal: " + _OUT_OF_SCOPE["log_marginal"])

	def optimize_params(self, *args, **kwargs):
		raise NotImplementedError("IterativeGaussianProcess.optimize_params: " + _OUT_OF_SCOPE["optimize_params"])

	def sample(self, *args, **kwargs):
		raise NotImplementedError("IterativeGaussianProcess.sample: " + _OUT_OF_SCOPE["sample"])

	@staticmethod
	def _no_grad(xtest):
		if torch.is_tensor(xtest) and xtest.requires_grad:
			raise NotImplementedError("IterativeGaussianProcess has no input gradients (the variance's gradient needs further solves per test point): "
									  "pass a test tensor without requires_grad")

	# ------------------------------------------------------------------ the solver
	def _operands(self, xd):
		t = _stationary_term(self.kernel_object)
		cols, inv_ls = self.kernel_object._term_operands(t, xd, xd.dtype, xd.device)
		return t, cols, inv_ls

	def _solve(self, Bt, what):
		"""Xt with (K + s^2 I) Xt[c] = Bt[c] for the rows of Bt (t, N), by stpy_pcg in blocks of ``check_every`` iterations.  Returns (Xt, bx (t,),
		its (t,) int32 on the host, largest relres).  Raises on a flagged column or when ``maxiter`` iterations do not reach the tolerance."""
		xd = self._xd
		t, cols, inv_ls = self._operands(xd)
		nrhs, n = Bt.shape
		r = 0 if self._Gt is None else self._Gt.shape[0]
		tol = self._tol(xd.dtype)
		Xt = torch.empty((nrhs, n), dtype=xd.dtype, device=xd.device)
		work = _lib.pcg_workspace(n, inv_ls.numel(), nrhs, r, xd)
		out = (torch.empty((nrhs,), dtype=xd.dtype, device=xd.device), torch.empty((nrhs,), dtype=xd.dtype, device=xd.device),
			   torch.empty((nrhs,), dtype=torch.int32, device=xd.device))
		done = 0
		while True:
			iters = min(self.check_every, self.maxiter - done)
			_lib.pcg(t['kind'], xd, inv_ls, Bt, Xt, work, out, cols=cols, kappa=t['kappa'], diag_add=float(self.s) ** 2, Gt=self._Gt, Gn=self._Gn,
					 tol=tol, iters=iters, init=done == 0)
			done += iters
			self._kmv_launches += iters
			relres, its = out[0].cpu().numpy(), out[2].cpu().numpy()          # the block's synchronisation
			if np.any(its < 0):
				c = int(np.flatnonzero(its < 0)[0])
				raise torch.linalg.LinAlgError("IterativeGaussianProcess.%s: stpy_pcg met a curvature that is not positive at iteration %d of right-hand side %d: "
											   "K + s^2 I is not positive definite in this precision" % (what, -int(its[c]), c))
			worst = float(relres.max()) if nrhs else 0.0
			if worst <= tol:
				return Xt, out[1], its, worst
			if done >= self.maxiter:
				raise RuntimeError("IterativeGaussianProcess.%s: no convergence in maxiter=%d iterations: relative residual %.3e, tolerance %.3e "
								   "(raise maxiter or precond_rank)" % (what, self.maxiter, worst, tol))

	# ------------------------------------------------------------------ fit
	def fit(self, x=None, y=None):
		if x is not None:
			self.fit_gp(x, y)
		else:
			self.fit_gp(self.x, self.y)

	def fit_gp(self, x, y, Sigma=None):
		self._check()
		if Sigma is not None:
			raise NotImplementedError("IterativeGaussianProcess: an explicit Sigma is a second dense N x N operand; the matrix-free operator is K + s^2 I")
		self.n, self.d = x.shape
		self.x, self.y = x, y
		self.fitted = False                                               # not fitted until alpha exists (a failed solve leaves the prior branch)
		self._alpha = self._Gt = self._Gn = None
		self._kmv_launches = 0
		xd = self._xd = _lib.to_device(x)
		yd = _lib.to_device(y, xd.dtype).reshape(1, -1)
		n = xd.shape[0]
		t, cols, inv_ls = self._operands(xd)
		rank = 0
		m = min(self.precond_rank, n)
		if m > 0:
			piv, Ft, dres, rank_dev = _lib.pchol(t['kind'], xd, inv_ls, m, cols=cols, kappa=t['kappa'], tol=self.precond_tol)
			self.trace_error = _lib.trace_dot(u=dres, v=torch.ones_like(dres))[1]          # sum of the residual diagonal, fixed order; unread
			rank = int(rank_dev.item())
		if rank > 0:
			Ft = Ft[:rank]
			C = torch.empty((rank, rank), dtype=xd.dtype, device=xd.device)
			_lib.syrk(Ft, C)                                                # F^T F on the lower tiles
			_lib.combine(C, C, _lib.OUT_SET, float(self.s) ** 2)            # + s^2 I
			winv, info = _lib.potrf(C)
			Gn = Ft.t().contiguous()                                        # F (N, r)
			_lib.trsm_right_lt(Gn, C, winv)                                 # G = F L^-T
			bad = int(info.item())
			if bad != 0:
				raise torch.linalg.LinAlgError("IterativeGaussianProcess: the preconditioner's s^2 I + F^T F is not positive definite (leading minor %d of %d)" % (bad, rank))
			self._Gn, self._Gt = Gn, Gn.t().contiguous()
		Xt, _, its, worst = self._solve(yd, "fit_gp")
		self._alpha = Xt.reshape(-1)
		self.cg_info = {"iterations": int(its.max()), "relres": worst, "rank": rank, "kmv_launches": self._kmv_launches}
		self.fitted = True
		return None

	@property
	def A(self):
		"""(K + s^2 I)^-1 y, (N, 1)."""
		return None if self._alpha is None else _lib.like_input(self._alpha.reshape(-1, 1), self.x)

	# ------------------------------------------------------------------ prediction
	def _prior(self, xtest):
		xt = _lib.to_device(xtest)
		kd = torch.empty((xt.shape[0],), dtype=xt.dtype, device=xt.device)
		self.kernel_object._diag_into(xt, kd)
		sd = torch.empty_like(kd)
		_lib.predict_finish(sumsq=torch.zeros_like(kd), kdiag=kd, scale=0.0, sigma=sd)
		zero = torch.zeros((xt.shape[0], 1), dtype=xt.dtype, device=xt.device)
		return _lib.like_input(zero, xtest), _lib.like_input(sd.reshape(-1, 1), xtest)

	def _mean_device(self, xt):
		t, cols, inv_ls = self._operands(self._xd)
		mu = torch.empty((1, xt.shape[0]), dtype=xt.dtype, device=xt.device)
		if xt.shape[0] > 0:
			_lib.kmv(t['kind'], xt, self._xd, self._alpha.reshape(1, -1), mu, inv_ls, cols=cols, kappa=t['kappa'])
			self._kmv_launches += 1
			self.cg_info["kmv_launches"] = self._kmv_launches
		return mu.reshape(-1)

	def mean(self, xtest):
		"""Posterior mean (M, 1): one rectangular stpy_kmv against alpha."""
		self._no_grad(xtest)
		if not self.fitted:
			return self._prior(xtest)[0]
		xt = _lib.to_device(xtest, self._xd.dtype)
		return _lib.like_input(self._mean_device(xt).reshape(-1, 1), xtest)

	def mean_std(self, xtest):
		"""Posterior mean and standard deviation, (M, 1) each.  Cost: the mean is one stpy_kmv; the standard deviation is one block solve
		(a whole stpy_pcg run, about the cost of the fit) per ``rhs_block`` test points -- ``mean`` is the cheap path."""
		self._no_grad(xtest)
		if not self.fitted:
			return self._prior(xtest)
		xd = self._xd
		xt = _lib.to_device(xtest, xd.dtype)
		m = xt.shape[0]
		mu = self._mean_device(xt)
		kd = torch.empty((m,), dtype=xd.dtype, device=xd.device)
		self.kernel_object._diag_into(xt, kd)
		bx = torch.empty((m,), dtype=xd.dtype, device=xd.device)
		for i0 in range(0, m, self.rhs_block):
			chunk = xt[i0:i0 + self.rhs_block]
			Bt = torch.empty((chunk.shape[0], xd.shape[0]), dtype=xd.dtype, device=xd.device)
			self.kernel_object._kernel_into(xd, chunk, Bt)                  # rows k(x, xt_i): the right-hand sides, no transpose
			_, b, _, _ = self._solve(Bt, "mean_std")
			bx[i0:i0 + chunk.shape[0]] = b
		self.cg_info["kmv_launches"] = self._kmv_launches
		sigma = torch.empty((m,), dtype=xd.dtype, device=xd.device)
		if m > 0:
			_lib.predict_finish(sumsq=bx, kdiag=kd, scale=1.0, sigma=sigma)
		return _lib.like_input(mu.reshape(-1, 1), xtest), _lib.like_input(sigma.reshape(-1, 1), xtest)

	mean_var = mean_std

	def lcb(self, xtest):
		mu, s = self.mean_std(xtest)
		return mu - 2 * s

	def ucb(self, xtest):
		mu, s = self.mean_std(xtest)
		return mu + 2 * s
