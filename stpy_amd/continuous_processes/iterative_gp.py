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

Out of scope, each for its own reason (what has an entry point raises NotImplementedError before the device is touched):
  log_marginal / optimize_params   the log-determinant of a matrix that is never formed needs stochastic Lanczos quadrature, an estimator with
                                   its own variance and probe count: a different contract from the exact evidence the other classes return;
  sample                           the reference's ``sample`` promises a draw of the exact posterior at the test points, which needs a square root of the
                                   N x N posterior covariance; the matrix-free draw lives in a finite Fourier basis of the prior and has its own
                                   name, ``sample_paths`` (below), as the stochastic evidence has;
  input gradients by autograd      (a test tensor with requires_grad) the analytic gradients have methods of their own, which return them
                                   directly: ``mean_std_grad`` (mean AND standard deviation; no solve beyond the one ``mean_std`` makes),
                                   ``mean_value_grad``, ``mean_value_grad_hessian`` and ``sample_paths`` (below);
  Hessians of pathwise samples     the prior term's second derivative (random features) has no kernel; the MEAN's Hessian is served (below);
  warm-started solves              between the L-BFGS steps of ``ucb_optimize`` every block solve starts from zero: stpy_pcg has no initial guess;
  Hessians beyond d = 16           stpy_kmv_dxx holds the selected coordinates in registers: at most 16 of them;
  composite kernels                the operator is evaluated inside the kernel for ONE stationary term (SE / Matern / ARD), the terms the pivoted
                                   Cholesky preconditioner covers as well;
  Sigma                            a general noise matrix is a second dense N x N operand;
  multi-GPU                        the row split of the operator needs its own reduction of the CG scalars across ranks.

That estimator exists under its own names, ``log_marginal_estimate`` and ``optimize_params_estimate`` (below): a randomised value with a reported
standard error, never returned where the exact evidence is asked for.

  log_marginal_estimate   stochastic Lanczos quadrature on the preconditioned operator.  Probes z_c = w1_c + F w2_c / s (covariance M, the
              preconditioner); ONE stpy_pcg_lanczos solve of the rows [y; z_1 .. z_t] gives alpha, u_c = A^-1 z_c and, per column, the CG scalars,
              which are the Lanczos coefficients: q_c = <z_c, M^-1 z_c> e_1^T (log T_c - log s^2 I) e_1 and
              log det A ~= mean_c q_c + (n - r) log s^2 + 2 sum log L_ll.  The last two terms are log det(s^2 I + F F^T), exact; the
              - log s^2 inside q_c is a control variate (it replaces the random <z, M^-1 z> log s^2 by its expectation n log s^2; without it
              the standard error is several times larger).  Gradient: -1/2 alpha^T dA alpha + 1/2 weight tr~, where tr~ estimates tr(A^-1 dA) =
              E[u_c^T dA v_c], v_c = M^-1 z_c, with the same idea as a control variate: b_c = v_c^T dA v_c / s^2 has the exactly known mean
              tr(P^-1 dA) = (tr dA - sum_l g_l^T dA g_l) / s^2 (P = s^2 I + F F^T, g_l the columns of G), and tr~ = mean(a) + beta (E b - mean(b))
              with the fitted beta (``_control_variate``).  Where the preconditioner is exact the random part vanishes in value AND gradient
              (an optimiser handed an exact value and a noisy slope stalls); where it is weak beta -> 0.  All bilinear forms come from
              stpy_kmv_dtheta: one pass over 1 + 2 t pairs and one over the r columns of G.  One evaluation with gradient = one stpy_pchol,
              one block solve of 1 + t columns, the derivative passes.  The standard error shrinks with 1 / sqrt(num_probes) and with the quality of the preconditioner: the
              probes only see what the rank-r factor leaves of K (large for a slowly decaying spectrum, e.g. Matern 5/2 at r << n).

Choosing the next point, matrix-free (csrc/kmvdx.hip, stpy_kmv_dx: values AND query-point gradients of sum_j V[c, j] k(x, x_j) for several rows c):

  mean_value_grad   (mu, d mu / dx) at the test points: ONE stpy_kmv_dx with Vt = alpha^T.
  sample_paths      pathwise conditioning (Matheron's rule): f_s(x) = phi(x)^T theta_s + k(x, X) v_s with v_s = A^-1 (y - Phi(X) theta_s - s eps_s),
              theta_s ~ N(0, I), eps_s ~ N(0, I), phi a random-Fourier basis of the prior (m / 2 frequencies W_j = (z_j tau_j) o inv_ls; tau = 1 for
              SE, sqrt(2 nu / u_j) with u_j ~ chi^2(2 nu) for Matern: the multivariate-t spectral density; cos and sin of the same frequency).
              The residual rows are built in row slabs of X (stpy_rff_embed, stpy_gemm_nt: Phi(X) is never stored whole), then ONE block solve
              per ``rhs_block`` draws.  The draw is exact GIVEN the basis -- its mean is the posterior mean and its variance the posterior
              variance of the model whose prior is the m-feature expansion, observed with noise s -- and the basis is the only approximation.
              The noise draw eps belongs to the rule: without it the variance of the draw is too small by s^2 |A^-1 k*|^2.
              The returned ``PathwiseSamples`` is a deterministic function with an analytic gradient: data term by stpy_kmv_dx, prior term by
              stpy_rff_grad, no further solve.
  sample_and_optimize   batch Thompson sampling: ``size`` paths from one block solve, each climbed from ``multistart`` starts, all of them one
              stacked L-BFGS-B problem with one batched device evaluation per step.

The deterministic acquisition, matrix-free.  With w = A^-1 k*(x) -- exactly the row of the block solve that ``mean_std`` makes for its variance --
    var(x) = k(x, x) - k*(x)^T w,     grad var(x) = grad k(x, x) - 2 sum_j w_j grad_x k(x, x_j)
(A^-1 is symmetric: both factors of the quadratic form give the same term), grad std = grad var / (2 std), 0 where std = 0.  No further solve:

  mean_std_grad     (d mu, d std), each (M, d): per ``rhs_block`` test points the block solve of ``mean_std``, its rows KEPT; d mu by stpy_kmv_dx, d std by
              the paired-weight form of stpy_gram_grad (KernelFunction._grad_into with Wt = the solve's rows, v = -1 / std) -- milliseconds
              beside the solve.  Memory O(M N) for the kept rows.
  ucb_optimize      GaussianProcess.ucb_optimize on this posterior: all starts one stacked L-BFGS-B problem, every evaluation
              ceil(multistart / rhs_block) block solves (each about one fit).
  mean_value_grad_hessian / mean_gradient_hessian   the mean, its input gradient and its input Hessian: ONE stpy_kmv_dxx (csrc/kmvdxx.hip) against
              alpha.  SE and Matern 5/2 (the second derivative of Matern 1/2 and 3/2 is singular at r = 0), at most 16 selected coordinates.
"""
import numpy as np
import scipy.linalg
import torch

from .. import _lib
from ..estimator import Estimator
from ..kernels import KernelFunction
from .nystrom_fea import _OVERRIDE_KEYS, _check_term_overrides, _stationary_term

_OUT_OF_SCOPE = {
	"log_marginal": "the log-determinant of a matrix that is never formed needs stochastic Lanczos quadrature (a randomised estimate, not the exact evidence)",
	"optimize_params": "it minimises log_marginal, whose log-determinant needs stochastic Lanczos quadrature here",
	"sample": "a posterior draw needs a square root of the N x N posterior covariance, which this class never forms",
}


class IterativeGaussianProcess(Estimator):

	def __init__(self, gamma=1, s=0.001, kappa=1., kernel_name="squared_exponential", d=1, kernel=None,
				 precond_rank=256, precond_tol=0., tol=None, maxiter=1000, check_every=10, rhs_block=64, nu=1.5, num_probes=16, probe_seed=0, bounds=None):
		self.s = s
		self.bounds = bounds
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
		self.num_probes, self.probe_seed = int(num_probes), int(probe_seed)
		self.evidence_info = None
		self.path_info = self.optimize_info = None
		self._probes = None
		self.trace_error = None
		self.cg_info = {"iterations": 0, "relres": 0.0, "rank": 0, "kmv_launches": 0}
		self._xd = self._alpha = self._Gt = self._Gn = None
		self._kmv_launches = 0
		self._solves = 0                                                  # block solves of the posterior variance (mean_std, mean_std_grad, ucb_optimize)
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
		if self.num_probes < 2:
			raise ValueError("IterativeGaussianProcess: num_probes must be at least 2 (the standard error is a sample standard deviation)")

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
			raise NotImplementedError("IterativeGaussianProcess returns its analytic input gradients directly (mean_std_grad, mean_value_grad, "
									  "mean_value_grad_hessian) instead of through autograd: pass a test tensor without requires_grad")

	# ------------------------------------------------------------------ the solver
	def _operands(self, xd):
		t = _stationary_term(self.kernel_object)
		cols, inv_ls = self.kernel_object._term_operands(t, xd, xd.dtype, xd.device)
		return t, cols, inv_ls

	def _solve(self, Bt, what, hyper=None, record=None):
		"""Xt with (K + s^2 I) Xt[c] = Bt[c] for the rows of Bt (t, N), by stpy_pcg in blocks of ``check_every`` iterations.  Returns (Xt, bx (t,),
		its (t,) int32 on the host, largest relres).  Raises on a flagged column or when ``maxiter`` iterations do not reach the tolerance.
		hyper: (term, cols, inv_ls, s, Gt, Gn) of another operator than the fitted one; record: (coef, rz0) for stpy_pcg_lanczos."""
		xd = self._xd
		if hyper is None:
			t, cols, inv_ls = self._operands(xd)
			s, Gt, Gn = float(self.s), self._Gt, self._Gn
		else:
			t, cols, inv_ls, s, Gt, Gn = hyper
		nrhs, n = Bt.shape
		r = 0 if Gt is None else Gt.shape[0]
		tol = self._tol(xd.dtype)
		Xt = torch.empty((nrhs, n), dtype=xd.dtype, device=xd.device)
		work = _lib.pcg_workspace(n, inv_ls.numel(), nrhs, r, xd)
		out = (torch.empty((nrhs,), dtype=xd.dtype, device=xd.device), torch.empty((nrhs,), dtype=xd.dtype, device=xd.device),
			   torch.empty((nrhs,), dtype=torch.int32, device=xd.device))
		done = 0
		while True:
			iters = min(self.check_every, self.maxiter - done)
			if record is None:
				_lib.pcg(t['kind'], xd, inv_ls, Bt, Xt, work, out, cols=cols, kappa=t['kappa'], diag_add=s ** 2, Gt=Gt, Gn=Gn,
						 tol=tol, iters=iters, init=done == 0)
			else:
				_lib.pcg_lanczos(t['kind'], xd, inv_ls, Bt, Xt, work, out, record[0], record[1], cols=cols, kappa=t['kappa'], diag_add=s ** 2, Gt=Gt, Gn=Gn,
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

	def _preconditioner(self, t, cols, inv_ls, s, probes_w2=None, Z=None):
		"""(rank, Gn, Gt, sum log L_ll (with Z only), trace word) of the rank <= precond_rank preconditioner for the given operands; with Z (t, N) and
		probes_w2 (t, >= rank) also Z += w2 F^T / s (one stpy_gemm_nt on the factor, before it is overwritten by G)."""
		xd = self._xd
		n = xd.shape[0]
		m = min(self.precond_rank, n)
		if m < 1:
			return 0, None, None, 0.0, None
		piv, Ft, dres, rank_dev = _lib.pchol(t['kind'], xd, inv_ls, m, cols=cols, kappa=t['kappa'], tol=self.precond_tol)
		trace = _lib.trace_dot(u=dres, v=torch.ones_like(dres))[1]            # sum of the residual diagonal, fixed order; unread
		rank = int(rank_dev.item())
		if rank < 1:
			return 0, None, None, 0.0, trace
		Ft = Ft[:rank]
		C = torch.empty((rank, rank), dtype=xd.dtype, device=xd.device)
		_lib.syrk(Ft, C)                                                # F^T F on the lower tiles
		_lib.combine(C, C, _lib.OUT_SET, s ** 2)                        # + s^2 I
		winv, info = _lib.potrf(C)
		Gn = Ft.t().contiguous()                                        # F (N, r)
		if Z is not None:
			_lib.gemm_nt((probes_w2[:, :rank] / s).contiguous(), Gn, Z, 2)
		_lib.trsm_right_lt(Gn, C, winv)                                 # G = F L^-T
		bad = int(info.item())
		if bad != 0:
			raise torch.linalg.LinAlgError("IterativeGaussianProcess: the preconditioner's s^2 I + F^T F is not positive definite (leading minor %d of %d)" % (bad, rank))
		sumlog = float(_lib.logdet_quad(C)[0].item()) if Z is not None else 0.0          # (the estimate's exact part; the fit has no use for it)
		return rank, Gn, Gn.t().contiguous(), sumlog, trace

	# ------------------------------------------------------------------ the stochastic evidence
	def _check_overrides(self, kernel, X):
		"""Host refusals of log_marginal_estimate; returns (X, the one stationary term it resolves to)."""
		return _check_term_overrides("IterativeGaussianProcess.log_marginal_estimate", "the matrix-free operator", self.kernel_object, kernel, X,
									 "'gamma' / 'ard_gamma'; the stored %s pass through unchanged" % ", ".join(repr(k) for k in _OVERRIDE_KEYS[2:]))

	def _probe_draws(self, n, dtype, device, probes):
		width = n + min(self.precond_rank, n)
		if probes is not None:
			W = torch.as_tensor(probes)
			if W.dim() != 2 or W.shape[0] < 2 or W.shape[1] < width:
				raise ValueError("IterativeGaussianProcess.log_marginal_estimate: probes must be (t >= 2, n + precond_rank = %d) standard normal draws, got %s"
								 % (width, tuple(W.shape)))
			return W.to(device=device, dtype=dtype)
		key = (n, width, self.num_probes, self.probe_seed, dtype)
		if self._probes is None or self._probes[0] != key:
			gen = torch.Generator(device="cpu").manual_seed(self.probe_seed)
			W = torch.randn((self.num_probes, width), generator=gen, dtype=torch.float64)
			self._probes = (key, W.to(device=device, dtype=dtype))          # drawn once per object and data size: common random numbers
		return self._probes[1]

	def log_marginal_estimate(self, kernel=None, X=None, weight=1.0, probes=None):
		"""A stochastic estimate of GaussianProcess.log_marginal's value 1/2 y^T A^-1 y + 1/2 weight log det A, A = K_theta + s^2 I, shape (1, 1),
		placed like the data (the module docstring states the estimator).  ``X``: overrides of the single kernel item, {'0': {'gamma' |
		'ard_gamma': tensor}}.  If a lengthscale tensor in ``X`` or ``self.s`` requires grad the result carries an autograd node whose backward is
		the estimated gradient.  Needs data (fit_gp); does its own stpy_pchol and solve for the hyper-parameters asked about and leaves the
		fitted state untouched.  ``probes``: (t, n + precond_rank) standard normal draws, columns [0, n) = w1, then w2; default: ``num_probes``
		rows drawn once from ``probe_seed`` and reused, so that the estimate is a deterministic function of the hyper-parameters.
		``self.evidence_info``: value, stderr, logdet, logdet_stderr, grad_stderr ({parameter name: array}, None without a gradient), probes,
		iterations, rank, kmv_launches, and q, the per-probe quadratures.  Standard errors are sample standard deviations / sqrt(t): they
		measure the probe variance, not the (much smaller) quadrature error."""
		kernel = self.kernel_object if kernel is None else kernel
		if self.num_probes < 2:
			raise ValueError("IterativeGaussianProcess: num_probes must be at least 2 (the standard error is a sample standard deviation)")
		X, term = self._check_overrides(kernel, X)
		if self.x is None or self.y is None:
			raise AttributeError("IterativeGaussianProcess.log_marginal_estimate needs data: call fit_gp first")
		params = self._grad_params(X, ("gamma", "ard_gamma"))
		if params:
			return _EstimateFn.apply(self, term, weight, probes, params, *[t for (_, _, t) in params])
		return self._estimate(term, weight, probes, [])[0]

	def _estimate(self, term, weight, probes, params):
		"""(value (1, 1), [gradient per entry of params])."""
		if self._xd is None:
			self._xd = _lib.to_device(self.x)
		xd = self._xd
		n = xd.shape[0]
		yd = _lib.to_device(self.y, xd.dtype).reshape(1, -1)
		s = float(self.s)
		w = float(weight.item()) if torch.is_tensor(weight) else float(weight)
		cols, inv_ls = self.kernel_object._term_operands(term, xd, xd.dtype, xd.device)
		W = self._probe_draws(n, xd.dtype, xd.device, probes)
		t = W.shape[0]
		Bt = torch.empty((1 + t, n), dtype=xd.dtype, device=xd.device)
		Bt[0] = yd[0]
		Bt[1:] = W[:, :n]
		rank, Gn, Gt, sumlog, _ = self._preconditioner(term, cols, inv_ls, s, probes_w2=W[:, n:], Z=Bt[1:])
		coef = torch.full((1 + t, self.maxiter, 2), float("nan"), dtype=torch.float64, device=xd.device)
		rz0 = torch.zeros((1 + t,), dtype=torch.float64, device=xd.device)
		launches = self._kmv_launches
		try:
			Xt, bx, its, worst = self._solve(Bt, "log_marginal_estimate", hyper=(term, cols, inv_ls, s, Gt, Gn), record=(coef, rz0))
		finally:
			used, self._kmv_launches = self._kmv_launches - launches, launches
		out = outg = None
		if params:
			# the derivative pass: rows [alpha; u_c; v_c] against rows [alpha; v_c; v_c], v_c = M^-1 z_c by the two NT products of the solver;
			# then the columns of G against themselves (the control variate's exact expectation)
			d = inv_ls.numel()
			Ut = torch.empty((1 + 2 * t, n), dtype=xd.dtype, device=xd.device)
			Vt = torch.empty((1 + 2 * t, n), dtype=xd.dtype, device=xd.device)
			Ut[:1 + t] = Xt
			Vt[0] = Xt[0]
			Vt[1:1 + t] = Bt[1:]
			if rank > 0:
				Wr = torch.empty((t, rank), dtype=xd.dtype, device=xd.device)
				_lib.gemm_nt(Bt[1:], Gt, Wr)
				_lib.gemm_nt(Wr, Gn, Vt[1:1 + t], 1)
			Vt[1 + t:] = Vt[1:1 + t]
			Ut[1 + t:] = Vt[1:1 + t]
			out = torch.empty((1 + 2 * t, d + 2), dtype=xd.dtype, device=xd.device)
			_lib.kmv_dtheta(term['kind'], xd, inv_ls, Ut, Vt, out, cols=cols, kappa=term['kappa'])
			used += 1
			outg = np.zeros((0, d + 2))
			if rank > 0:
				og = torch.empty((rank, d + 2), dtype=xd.dtype, device=xd.device)
				_lib.kmv_dtheta(term['kind'], xd, inv_ls, Gt, Gt, og, cols=cols, kappa=term['kappa'])
				used += 1
				outg = og.double().cpu().numpy()
			out = out.double().cpu().numpy()
		# host: at most 1 + t tridiagonal eigenproblems of order its
		coef_h, rz0_h, yalpha = coef[1:].cpu().numpy(), rz0[1:].cpu().numpy(), float(bx[0].item())
		q = np.zeros(t)
		for c in range(t):
			m = int(its[1 + c])
			if m < 1:
				continue                                                   # (a zero probe: q = 0)
			a, b = coef_h[c, :m, 0], coef_h[c, :m - 1, 1]
			dg = 1.0 / a
			dg[1:] += b / a[:-1]
			if m > 1:
				theta, V = scipy.linalg.eigh_tridiagonal(dg, np.sqrt(b) / a[:-1], lapack_driver="stev")          # (QR iteration: the default MRRR driver gave up on the clustered Ritz values of an 800-step run)
				q[c] = rz0_h[c] * float(np.sum(V[0] ** 2 * (np.log(theta) - np.log(s * s))))
			else:
				q[c] = rz0_h[c] * (np.log(dg[0]) - np.log(s * s))
		sem = lambda v: float(np.std(v, ddof=1) / np.sqrt(len(v)))
		logdet = float(q.mean()) + (n - rank) * np.log(s * s) + 2.0 * sumlog
		value = 0.5 * yalpha + 0.5 * w * logdet
		grads, gse = [], None
		if params:
			il = np.asarray(term['inv_ls'], dtype=np.float64)
			gse = {}
			for (key, name, tensor) in params:
				if key == "likelihood":                                     # dA/ds = 2 s I; tr(P^-1) = (n - |G|_F^2) / s^2
					rows, rowsg, tr_dA = 2.0 * s * out[:, d + 1:d + 2], 2.0 * s * outg[:, d + 1:d + 2], np.array([2.0 * s * n])
					shown = "sigma"
				else:
					if term['pname'] != name:
						raise NotImplementedError("IterativeGaussianProcess.log_marginal_estimate: the kernel has no '%s' lengthscale" % name)
					# d/d gamma_p = sum over the coordinates k that gamma_p scales of (out[c, k] / inv_ls[k]) * (-inv_ls[k]^2); tr(dK/dgamma) = 0
					rows, rowsg = np.zeros((1 + 2 * t, tensor.numel())), np.zeros((outg.shape[0], tensor.numel()))
					for k, pk in enumerate(term['pidx']):
						rows[:, int(pk)] -= out[:, k] * il[k]
						rowsg[:, int(pk)] -= outg[:, k] * il[k]
					tr_dA, shown = np.zeros(rows.shape[1]), name
				g, se = np.zeros(rows.shape[1]), np.zeros(rows.shape[1])
				for j in range(rows.shape[1]):
					tr, se_j = _control_variate(rows[1:1 + t, j], rows[1 + t:, j] / (s * s), (tr_dA[j] - rowsg[:, j].sum()) / (s * s))
					g[j], se[j] = -0.5 * rows[0, j] + 0.5 * w * tr, 0.5 * w * se_j
				gse[shown] = se
				grads.append(torch.from_numpy(g).reshape(tensor.shape if tensor.dim() > 0 else ()).to(device=tensor.device, dtype=tensor.dtype))
		self.evidence_info = {"value": value, "stderr": 0.5 * w * sem(q), "logdet": logdet, "logdet_stderr": sem(q), "grad_stderr": gse, "probes": t,
							  "iterations": int(its.max()), "rank": rank, "kmv_launches": used, "q": q}
		val = torch.full((1, 1), value, dtype=xd.dtype, device=xd.device)
		return _lib.like_input(val, self.x), grads

	def optimize_params_estimate(self, type='bandwidth', restarts=10, regularizer=None, maxiter=1000, mingradnorm=1e-4, verbose=False,
								 optimizer="pytorch-minimize", scale=1., weight=1., save=False, save_name='model.np', init_func=None, bounds=None,
								 parallel=False, cores=None):
		"""GaussianProcess.optimize_params with ``log_marginal_estimate`` for the objective: the same parameter dictionary ('gamma' / 'ard_gamma'
		of the item, with "bandwidth+noise" also the noise std) through Estimator.optimize_params_general, which writes the best point back
		and refits.  ``parallel=True`` is accepted and runs serially.
		The probes are fixed (common random numbers), so the objective is a deterministic function; but the value estimate and the gradient
		estimate are two estimators of neighbouring quantities, not an exact derivative pair: a line search can stall where they disagree by
		more than the decrease it asks for.  Raise ``num_probes`` or ``precond_rank`` (both shrink the standard errors in ``evidence_info``)
		when that happens."""
		if type not in ("bandwidth", "bandwidth+noise"):
			raise NotImplementedError("IterativeGaussianProcess.optimize_params_estimate(type='%s'): 'bandwidth' and 'bandwidth+noise' only" % type)
		if regularizer is not None:
			raise NotImplementedError("IterativeGaussianProcess.optimize_params_estimate: no regularizer")
		params = self._bandwidth_params(type, init_func, bounds)
		view = _EstimateView.__new__(_EstimateView)
		view.__dict__ = self.__dict__                                       # the same state: what the driver writes lands on this object
		return view.optimize_params_general(params=params, restarts=restarts, optimizer=optimizer, maxiter=maxiter, mingradnorm=mingradnorm,
											verbose=verbose, scale=scale, weight=weight, save=save, save_name=save_name, parallel=False, cores=cores)

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
		t, cols, inv_ls = self._operands(xd)
		rank, self._Gn, self._Gt, _, self.trace_error = self._preconditioner(t, cols, inv_ls, float(self.s))
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
		mu, sigma, _ = self._mean_std_device(_lib.to_device(xtest, self._xd.dtype), "mean_std")
		return _lib.like_input(mu.reshape(-1, 1), xtest), _lib.like_input(sigma.reshape(-1, 1), xtest)

	def _mean_std_device(self, xt, what, keep=False):
		"""mu, sigma (M,) for device test points and, with ``keep``, the rows w_i = A^-1 k*_i of the block solves as Wt (M, N) (else None): what the
		variance's input gradient is made of, computed anyway and otherwise dropped."""
		xd = self._xd
		m = xt.shape[0]
		mu = self._mean_device(xt)
		kd = torch.empty((m,), dtype=xd.dtype, device=xd.device)
		self.kernel_object._diag_into(xt, kd)
		bx = torch.empty((m,), dtype=xd.dtype, device=xd.device)
		Wt = torch.empty((m, xd.shape[0]), dtype=xd.dtype, device=xd.device) if keep else None
		for i0 in range(0, m, self.rhs_block):
			chunk = xt[i0:i0 + self.rhs_block]
			Bt = torch.empty((chunk.shape[0], xd.shape[0]), dtype=xd.dtype, device=xd.device)
			self.kernel_object._kernel_into(xd, chunk, Bt)                  # rows k(x, xt_i): the right-hand sides, no transpose
			Xt, b, _, _ = self._solve(Bt, what)
			bx[i0:i0 + chunk.shape[0]] = b
			if keep:
				Wt[i0:i0 + chunk.shape[0]] = Xt
			self._solves += 1
		self.cg_info["kmv_launches"] = self._kmv_launches
		sigma = torch.empty((m,), dtype=xd.dtype, device=xd.device)
		if m > 0:
			_lib.predict_finish(sumsq=bx, kdiag=kd, scale=1.0, sigma=sigma)
		return mu, sigma, Wt

	mean_var = mean_std

	def lcb(self, xtest):
		mu, s = self.mean_std(xtest)
		return mu - 2 * s

	def ucb(self, xtest):
		mu, s = self.mean_std(xtest)
		return mu + 2 * s

	# ------------------------------------------------------------------ input gradients of the posterior, Hessian of the mean
	def _posterior(self, xtest):
		"""mu, sigma (M,) on the device and what their input gradient needs: (xt, Wt or None, sigma), Wt (M, N) the kept rows A^-1 k*_i (the shapes of
		GaussianProcess._posterior).  Costs ceil(M / rhs_block) block solves."""
		if not self.fitted:
			xt = _lib.to_device(xtest)
			kd = torch.empty((xt.shape[0],), dtype=xt.dtype, device=xt.device)
			self.kernel_object._diag_into(xt, kd)
			sigma = torch.empty_like(kd)
			_lib.predict_finish(sumsq=torch.zeros_like(kd), kdiag=kd, scale=0.0, sigma=sigma)
			return torch.zeros_like(kd), sigma, (xt, None, sigma)
		xt = _lib.to_device(xtest, self._xd.dtype)
		mu, sigma, Wt = self._mean_std_device(xt, "mean_std_grad", keep=True)
		return mu, sigma, (xt, Wt, sigma)

	def _posterior_grad(self, state, gmu, gstd):
		"""sum_t gmu_t grad mu(xt_t) + gstd_t grad sigma(xt_t), one row per test point: (M, d) on the device, no solve.  grad mu: one stpy_kmv_dx
		against alpha.  grad sigma = (grad_x k(x, x) - 2 sum_j w_j grad_x k(x, x_j)) / (2 sigma), 0 where sigma is 0: the paired-weight
		stpy_gram_grad with the kept rows w and v = -gstd / sigma, plus KernelFunction._self_grad_into (zero for the stationary terms served here)."""
		xt, Wt, sigma = state
		ko = self.kernel_object
		G = torch.zeros(xt.shape, dtype=xt.dtype, device=xt.device)
		m = xt.shape[0]
		if m == 0:
			return G
		u = None if gmu is None else _lib.to_device(gmu, xt.dtype).reshape(-1)
		gs = None if gstd is None else _lib.to_device(gstd, xt.dtype).reshape(-1)
		if gs is not None and not bool((gs != 0).any()):
			gs = None
		if Wt is not None and u is not None:
			t, cols, inv_ls = self._operands(self._xd)
			dsel = inv_ls.numel()
			out = torch.empty((1, m, dsel + 1), dtype=xt.dtype, device=xt.device)
			_lib.kmv_dx(t['kind'], xt, self._xd, self._alpha.reshape(1, -1), out, inv_ls, cols=cols, kappa=t['kappa'])
			self._kmv_launches += 1
			self.cg_info["kmv_launches"] = self._kmv_launches
			G[:, t['group']] = u.reshape(-1, 1) * out[0, :, :dsel]
		if gs is not None:
			pos = sigma > 0
			safe = torch.where(pos, sigma, torch.ones_like(sigma))
			if Wt is not None:
				v = torch.where(pos, -gs / safe, torch.zeros_like(gs)).contiguous()
				Gs = torch.zeros_like(G)
				ko._grad_into(self._xd, xt, Gs, Wt=Wt, v=v)
				G += Gs
			ko._self_grad_into(xt, torch.where(pos, gs / (2.0 * safe), torch.zeros_like(gs)), G)
		return G

	def mean_std_grad(self, xtest):
		"""Batched input gradients of the posterior: (d mu, d std), each (M, d), where the inputs live (GaussianProcess.mean_std_grad).  Cost: the
		block solves of ``mean_std`` on the same points -- the rows w_i = A^-1 k*_i they produce ARE the coefficients of the variance's gradient --
		and two cheap passes over the points.  Not fitted: zeros (the prior of a stationary kernel is flat)."""
		xtest = torch.as_tensor(xtest).detach()
		m = xtest.shape[0]
		if not self.fitted:
			dt = xtest.dtype if xtest.dtype in (torch.float32, torch.float64) else torch.float64
			return torch.zeros((m, self.d), dtype=dt, device=xtest.device), torch.zeros((m, self.d), dtype=dt, device=xtest.device)
		mu, sigma, state = self._posterior(xtest)
		ones = torch.ones_like(sigma)
		dmu = self._posterior_grad(state, ones, None)
		dstd = self._posterior_grad(state, None, ones)
		return _lib.like_input(dmu, xtest), _lib.like_input(dstd, xtest)

	def ucb_optimize(self, beta, multistart=25, lcb=False):
		"""GaussianProcess.ucb_optimize, matrix-free: maximise mu + sqrt(beta) sigma (mu - sqrt(beta) sigma with ``lcb``) over ``self.bounds`` from
		``multistart`` uniform starts drawn with the reference's np.random calls in its order.  All starts are ONE stacked L-BFGS-B problem
		(``_multistart_maximize`` of gauss_procc.py); every evaluation is ceil(multistart / rhs_block) block solves, each about the cost of the
		fit, and the analytic gradients come out of the same solves.  Returns (solution (d,), value) of the best start, never below the
		acquisition at any drawn start.  ``self.optimize_info``: starts, start_values, evaluations, solves (= evaluations * ceil(multistart / rhs_block)),
		kmv_launches."""
		from .gauss_procc import _draw_starts, _multistart_maximize
		if self.bounds is None:
			raise ValueError("ucb_optimize needs box bounds: set IterativeGaussianProcess.bounds to a list of (low, high) per coordinate")
		multistart = int(multistart)
		if multistart < 1:
			raise ValueError("IterativeGaussianProcess.ucb_optimize: multistart=%d must be at least 1" % multistart)
		bounds = tuple((float(a), float(b)) for (a, b) in self.bounds)
		if len(bounds) != self.d:
			raise ValueError("IterativeGaussianProcess.ucb_optimize: %d bounds for d=%d" % (len(bounds), self.d))
		starts = _draw_starts(multistart, self.d, bounds)
		sign, sb = (-1.0 if lcb else 1.0), float(np.sqrt(beta))
		dev = self._xd.device if self._xd is not None else _lib.device()
		dtype = self._xd.dtype if self._xd is not None else torch.float64
		solves, launches = self._solves, self._kmv_launches
		first = []

		def value(xt):
			mu, sigma, state = self._posterior(xt)
			val = mu + sign * sb * sigma
			if not first:
				first.append(val.double().cpu().numpy())                    # the first evaluation is at the drawn starts
			return val, state

		def evaluate(xt):
			val, state = value(xt)
			return val, self._posterior_grad(state, torch.ones_like(val), torch.full_like(val, sign * sb))

		sol, vals, evals = _multistart_maximize(evaluate, starts, bounds, dev, dtype, final=lambda xt: value(xt)[0])
		x0, v0 = np.asarray(starts, dtype=np.float64), first[0]
		keep = v0 > vals                                                   # the line search watches the SUM: a start its climb did not improve stays
		sol[keep], vals[keep] = x0[keep], v0[keep]
		index = int(np.argmax(vals))
		self.optimize_info = {"starts": x0, "start_values": v0, "evaluations": evals, "solves": self._solves - solves,
							  "kmv_launches": self._kmv_launches - launches}
		return (torch.from_numpy(sol[index].copy()), torch.tensor(float(vals[index]), dtype=torch.float64))

	def _hessian_refusal(self):
		"""The dense class's refusal (KernelFunction._grad_into), on the host."""
		t = _stationary_term(self.kernel_object)
		if t['kind'] in (_lib.K_MATERN12, _lib.K_MATERN32):
			raise NotImplementedError("Hessian of the %s term is not defined (singular at r = 0)" % self.kernel_object._term_name(t))
		if len(t['group']) > 16:
			raise NotImplementedError("IterativeGaussianProcess: the matrix-free Hessian (stpy_kmv_dxx) serves at most 16 selected coordinates, the kernel reads %d"
									  % len(t['group']))
		return t

	def mean_value_grad_hessian(self, xtest):
		"""Posterior mean (M, 1), its input gradient (M, d) and its input Hessian (M, d, d), symmetric and scattered to the full d (zero on the
		coordinates the kernel does not read): ONE stpy_kmv_dxx against alpha.  Not fitted: zeros.  SE and Matern 5/2, at most 16 selected coordinates."""
		self._no_grad(xtest)
		self._hessian_refusal()
		xtest = torch.as_tensor(xtest)
		m = xtest.shape[0]
		if not self.fitted:
			dt = xtest.dtype if xtest.dtype in (torch.float32, torch.float64) else torch.float64
			z = lambda *shape: torch.zeros(shape, dtype=dt, device=xtest.device)
			return z(m, 1), z(m, self.d), z(m, self.d, self.d)
		xd = self._xd
		xt = _lib.to_device(xtest, xd.dtype)
		t, cols, inv_ls = self._operands(xd)
		dsel, width = inv_ls.numel(), xd.shape[1]
		out = torch.zeros((1, m, _lib.kmv_dxx_ncol(dsel)), dtype=xd.dtype, device=xd.device)
		if m > 0:
			_lib.kmv_dxx(t['kind'], xt, xd, self._alpha.reshape(1, -1), out, inv_ls, cols=cols, kappa=t['kappa'])
			self._kmv_launches += 1
			self.cg_info["kmv_launches"] = self._kmv_launches
		group = torch.as_tensor(t['group'], dtype=torch.long, device=xd.device)
		grad = torch.zeros((m, width), dtype=xd.dtype, device=xd.device)
		grad[:, group] = out[0, :, :dsel]
		# the lower triangle, row by row, to both halves of the full matrix: the two copies of an entry are the same bits
		rows, colsl = torch.tril_indices(dsel, dsel, device=xd.device)
		H = torch.zeros((m, width, width), dtype=xd.dtype, device=xd.device)
		tri = out[0, :, dsel + 1:]
		H[:, group[rows], group[colsl]] = tri
		H[:, group[colsl], group[rows]] = tri
		return _lib.like_input(out[0, :, dsel].reshape(-1, 1).clone(), xtest), _lib.like_input(grad, xtest), _lib.like_input(H, xtest)

	def mean_gradient_hessian(self, xtest, hessian=False):
		"""The reference's convention (GaussianProcess.mean_gradient_hessian): the gradient (d,) of the posterior mean at the FIRST row of xtest,
		and with ``hessian`` [gradient, Hessian (d, d)].  One stpy_kmv_dxx launch against alpha (one stpy_kmv_dx without the Hessian)."""
		self._no_grad(xtest)
		x1 = xtest[:1].detach() if torch.is_tensor(xtest) else torch.as_tensor(xtest[:1])
		if hessian:
			_, g, H = self.mean_value_grad_hessian(x1)
			return [g[0], H[0]]
		return self.mean_value_grad(x1)[1][0]

	# ------------------------------------------------------------------ input gradients and pathwise samples
	def mean_value_grad(self, xtest):
		"""Posterior mean (M, 1) and its input gradient (M, d): ONE stpy_kmv_dx against alpha.  Not fitted: zeros (the prior mean)."""
		self._no_grad(xtest)
		xtest = torch.as_tensor(xtest)
		m = xtest.shape[0]
		if not self.fitted:
			dt = xtest.dtype if xtest.dtype in (torch.float32, torch.float64) else torch.float64
			return torch.zeros((m, 1), dtype=dt, device=xtest.device), torch.zeros((m, self.d), dtype=dt, device=xtest.device)
		xd = self._xd
		xt = _lib.to_device(xtest, xd.dtype)
		t, cols, inv_ls = self._operands(xd)
		dsel = inv_ls.numel()
		out = torch.zeros((1, m, dsel + 1), dtype=xd.dtype, device=xd.device)
		if m > 0:
			_lib.kmv_dx(t['kind'], xt, xd, self._alpha.reshape(1, -1), out, inv_ls, cols=cols, kappa=t['kappa'])
			self._kmv_launches += 1
			self.cg_info["kmv_launches"] = self._kmv_launches
		grad = out[0, :, :dsel]
		if cols is not None:
			full = torch.zeros((m, xd.shape[1]), dtype=xd.dtype, device=xd.device)
			full[:, t['group']] = grad
			grad = full
		return _lib.like_input(out[0, :, dsel].reshape(-1, 1).clone(), xtest), _lib.like_input(grad.clone(), xtest)

	_DRAW_KEYS = ("z", "u", "theta", "eps")

	def _path_draws(self, term, size, m, n, draws, seed):
		"""The standard normal (u: chi-square) draws of sample_paths as float64 CPU tensors, shapes checked: z (m / 2, coordinates of the term),
		u (m / 2,) for a Matern term (else None), theta (size, m), eps (size, n).  Default: a CPU generator seeded by ``seed``, in this order."""
		dsel, two_nu = len(term['group']), _TWO_NU.get(term['kind'])
		shapes = {"z": (m // 2, dsel), "u": (m // 2,), "theta": (size, m), "eps": (size, n)}
		given = {} if draws is None else dict(draws)
		for key in given:
			if key not in self._DRAW_KEYS:
				raise ValueError("IterativeGaussianProcess.sample_paths: draws has the unknown entry %r (known: 'z', 'u', 'theta', 'eps')" % (key,))
		gen = torch.Generator(device="cpu").manual_seed(int(seed))
		out = {}
		for key in self._DRAW_KEYS:
			if key == "u" and two_nu is None:
				if given.get("u") is not None:
					raise ValueError("IterativeGaussianProcess.sample_paths: draws['u'] belongs to a Matern kernel; the squared exponential has no radial mixing")
				out["u"] = None
				continue
			if given.get(key) is not None:
				v = torch.as_tensor(given[key]).detach().to(device="cpu", dtype=torch.float64)
				if tuple(v.shape) != shapes[key]:
					raise ValueError("IterativeGaussianProcess.sample_paths: draws[%r] must have shape %s, got %s" % (key, shapes[key], tuple(v.shape)))
				if key == "u" and not bool((v > 0).all()):
					raise ValueError("IterativeGaussianProcess.sample_paths: draws['u'] must be positive (chi-square draws)")
			elif key == "u":
				v = (torch.randn((m // 2, two_nu), generator=gen, dtype=torch.float64) ** 2).sum(dim=1)
			else:
				v = torch.randn(shapes[key], generator=gen, dtype=torch.float64)
			out[key] = v
		return out

	def sample_paths(self, size=1, num_features=2048, seed=0, draws=None):
		"""``size`` posterior draws by pathwise conditioning, as a ``PathwiseSamples`` function object (the module docstring states the rule).
		num_features: m, even; the prior basis has m / 2 frequencies.  draws: {'z', 'u', 'theta', 'eps'} standard normal (u: chi-square with 2 nu
		degrees of freedom) arrays that replace the seeded ones, so that an oracle can share them.  One block solve per ``rhs_block`` draws;
		memory O(size N + slab m).  ``self.path_info``: iterations, relres, kmv_launches, features."""
		term = _stationary_term(self.kernel_object)
		size, m = int(size), int(num_features)
		if size < 1:
			raise ValueError("IterativeGaussianProcess.sample_paths: size=%d must be at least 1" % size)
		if m < 2 or m % 2:
			raise ValueError("IterativeGaussianProcess.sample_paths: num_features=%d must be even and positive (cos and sin of every frequency)" % m)
		if not self.fitted or self.x is None:
			raise AttributeError("IterativeGaussianProcess.sample_paths needs a fitted object: call fit_gp first")
		n = self.x.shape[0]
		dr = self._path_draws(term, size, m, n, draws, seed)
		xd = self._xd
		dt, dev = xd.dtype, xd.device
		_, cols, inv_ls = self._operands(xd)
		# the basis: W_j = (z_j tau_j) o inv_ls on the term's columns, stacked twice (cos | sin of the same frequency)
		tau = torch.ones((m // 2, 1), dtype=torch.float64) if dr["u"] is None else torch.sqrt(float(_TWO_NU[term['kind']]) / dr["u"]).reshape(-1, 1)
		Wh = torch.zeros((m // 2, xd.shape[1]), dtype=torch.float64)
		Wh[:, term['group']] = dr["z"] * tau * torch.as_tensor(np.asarray(term['inv_ls'], dtype=np.float64)).reshape(1, -1)
		W = torch.cat([Wh, Wh], dim=0).to(device=dev, dtype=dt)
		scale = float(np.sqrt(2.0 / m) * np.sqrt(float(term['kappa'])))
		theta = dr["theta"].to(device=dev, dtype=dt)
		# residual rows R = 1 y^T - s eps - theta Phi(X)^T, in row slabs of X
		R = dr["eps"].to(device=dev, dtype=dt)
		R.mul_(-float(self.s)).add_(_lib.to_device(self.y, dt).reshape(1, -1))
		slab = max(64, min(n, (1 << 24) // m))
		for i0 in range(0, n, slab):
			Phi = _lib.rff_embed(xd[i0:i0 + slab], W, m, scale)
			T = torch.empty((size, Phi.shape[0]), dtype=dt, device=dev)
			_lib.gemm_nt(theta, Phi, T)
			R[:, i0:i0 + slab] -= T
		V = torch.empty((size, n), dtype=dt, device=dev)
		launches, its_max, worst = self._kmv_launches, 0, 0.0
		for b0 in range(0, size, self.rhs_block):
			Xt, _, its, rel = self._solve(R[b0:b0 + self.rhs_block], "sample_paths")
			V[b0:b0 + self.rhs_block] = Xt
			its_max, worst = max(its_max, int(its.max())), max(worst, rel)
		self.cg_info["kmv_launches"] = self._kmv_launches
		self.path_info = {"iterations": its_max, "relres": worst, "kmv_launches": self._kmv_launches - launches, "features": m}
		return PathwiseSamples(xd, term, cols, inv_ls, W, scale, theta, V, self.x)

	def sample_and_optimize(self, size=1, multistart=25, bounds=None, num_features=2048, seed=0):
		"""Batch Thompson sampling: ``size`` paths from one block solve (``sample_paths``), each maximised over the box ``bounds`` (default: the
		bounding box of the training points) from ``multistart`` uniform starts.  All size * multistart points are ONE stacked L-BFGS-B problem with
		one batched device evaluation per step (``_multistart_maximize`` of gauss_procc.py; the starts come from np.random as there).  Returns
		(solutions (size, d), values (size,)): the best climbed start of every path, never below the path's value at any of its starts.  ``self.optimize_info``: starts, evaluations."""
		from .gauss_procc import _draw_starts, _multistart_maximize
		size, multistart = int(size), int(multistart)
		if multistart < 1:
			raise ValueError("IterativeGaussianProcess.sample_and_optimize: multistart=%d must be at least 1" % multistart)
		paths = self.sample_paths(size=size, num_features=num_features, seed=seed)
		xd = self._xd
		d = xd.shape[1]
		if bounds is None:
			lo, hi = xd.min(dim=0)[0].double().cpu().numpy(), xd.max(dim=0)[0].double().cpu().numpy()
			bounds = tuple((float(a), float(b)) for a, b in zip(lo, hi))
		bounds = tuple((float(a), float(b)) for (a, b) in bounds)
		if len(bounds) != d:
			raise ValueError("IterativeGaussianProcess.sample_and_optimize: %d bounds for d=%d" % (len(bounds), d))
		starts = _draw_starts(size * multistart, d, bounds)
		which = torch.arange(size, device=xd.device).repeat_interleave(multistart)
		evaluate = lambda xt: paths._value_grad_device(xt, which)
		x0 = np.asarray(starts, dtype=np.float64)
		v0 = evaluate(torch.from_numpy(x0).to(device=xd.device, dtype=xd.dtype))[0].double().cpu().numpy()
		sol, vals, evals = _multistart_maximize(evaluate, starts, bounds, xd.device, xd.dtype)
		keep = v0 > vals                                                   # the line search watches the SUM: a start its climb did not improve stays
		sol[keep], vals[keep] = x0[keep], v0[keep]
		sol, vals = sol.reshape(size, multistart, d), vals.reshape(size, multistart)
		best = np.argmax(vals, axis=1)
		self.optimize_info = {"starts": np.asarray(starts).reshape(size, multistart, d), "evaluations": evals + 1, "paths": paths}
		pick = np.arange(size)
		return (_lib.like_input(torch.from_numpy(sol[pick, best].copy()).to(device=xd.device, dtype=xd.dtype), self.x),
				_lib.like_input(torch.from_numpy(vals[pick, best].copy()).to(device=xd.device, dtype=xd.dtype), self.x))


_TWO_NU = {_lib.K_MATERN12: 1, _lib.K_MATERN32: 3, _lib.K_MATERN52: 5}          # degrees of freedom of the multivariate-t spectral density


class PathwiseSamples:
	"""``size`` posterior draws of an IterativeGaussianProcess as deterministic functions: f_s(x) = phi(x)^T theta_s + k(x, X) v_s.  Calling the
	object returns the values (M, size); ``value_grad`` also the input gradients.  The data term is ONE stpy_kmv_dx against the rows v_s; the
	prior term is stpy_rff_grad with per-point coefficient rows, added into the same result.  No solve, and no host synchronisation beyond
	the result.  The object keeps what it needs (points, basis, theta, v) and does not change when the estimator is refitted."""

	CHUNK = 256          # points per stpy_rff_grad launch, always this many (padded): a point's bits do not depend on how many points ride with it

	def __init__(self, xd, term, cols, inv_ls, W, scale, theta, V, ref):
		self._xd, self._term, self._cols, self._inv_ls = xd, term, cols, inv_ls
		self._W, self._scale, self._theta, self._V, self._ref = W, scale, theta, V, ref
		self.size, self.num_features, self.d = V.shape[0], W.shape[0], xd.shape[1]

	def _value_grad_device(self, xt, which=None):
		"""Device in, device out: (values, gradients) as (M, size), (M, size, d), or with which (M,) as (M,), (M, d)."""
		xd, dsel, size, m, d = self._xd, self._inv_ls.numel(), self.size, self.num_features, self.d
		dt, dev = xd.dtype, xd.device
		M = xt.shape[0]
		out = torch.zeros((size, M, dsel + 1), dtype=dt, device=dev)
		if M > 0:
			_lib.kmv_dx(self._term['kind'], xt, xd, self._V, out, self._inv_ls, cols=self._cols, kappa=self._term['kappa'])
		if which is None:
			data = out.permute(1, 0, 2).reshape(M * size, dsel + 1)          # stacked point p = i * size + s
			pts = xt.repeat_interleave(size, dim=0)
			idx = torch.arange(size, device=dev).repeat(M)
		else:
			idx = which.to(device=dev, dtype=torch.long)
			data = out[idx, torch.arange(M, device=dev)]
			pts = xt
		S = pts.shape[0]
		val = torch.empty((S,), dtype=dt, device=dev)
		G = torch.empty((S, d), dtype=dt, device=dev)
		group = self._term['group']
		for p0 in range(0, S, self.CHUNK):
			k = min(self.CHUNK, S - p0)
			xc = torch.zeros((self.CHUNK, d), dtype=dt, device=dev)
			xc[:k] = pts[p0:p0 + k]
			C = torch.zeros((self.CHUNK, m), dtype=dt, device=dev)
			C[:k] = self._theta[idx[p0:p0 + k]]
			vc = torch.zeros((self.CHUNK,), dtype=dt, device=dev)
			Gc = torch.zeros((self.CHUNK, d), dtype=dt, device=dev)
			vc[:k] = data[p0:p0 + k, dsel]
			Gc[:k, group] = data[p0:p0 + k, :dsel]
			_lib.rff_grad(xc, self._W, m, self._scale, C, Gc, val=vc, combine=_lib.OUT_ADD)          # the prior term adds into the data term
			val[p0:p0 + k] = vc[:k]
			G[p0:p0 + k] = Gc[:k]
		if which is None:
			return val.reshape(M, size), G.reshape(M, size, d)
		return val, G

	def value_grad(self, xtest, which=None):
		"""((M, size), (M, size, d)) values and input gradients of every path at every test point; with ``which`` (M,) integers, point i on path
		which[i] only: ((M,), (M, d)), the matching entries of the full call bit for bit."""
		if torch.is_tensor(xtest) and xtest.requires_grad:
			raise NotImplementedError("PathwiseSamples.value_grad returns the analytic gradient itself: pass a test tensor without requires_grad")
		xtest = torch.as_tensor(xtest)
		if xtest.dim() != 2 or xtest.shape[1] != self.d:
			raise ValueError("PathwiseSamples: test points must be (M, %d), got %s" % (self.d, tuple(xtest.shape)))
		if which is not None:
			which = torch.as_tensor(which)
			if which.dim() != 1 or which.shape[0] != xtest.shape[0] or which.dtype.is_floating_point:
				raise ValueError("PathwiseSamples.value_grad: which must be (M,) = (%d,) integers, got %s %s" % (xtest.shape[0], tuple(which.shape), which.dtype))
			if which.numel() and (int(which.min()) < 0 or int(which.max()) >= self.size):
				raise IndexError("PathwiseSamples.value_grad: which outside [0, %d)" % self.size)
		val, G = self._value_grad_device(_lib.to_device(xtest, self._xd.dtype), which)
		return _lib.like_input(val, xtest), _lib.like_input(G, xtest)

	def __call__(self, xtest):
		return self.value_grad(xtest)[0]


def _control_variate(a, b, Eb):
	"""(estimate, standard error) of E[a] from paired samples a_c = u_c^T dA v_c and b_c = v_c^T dA v_c / s^2 with E[b] = tr(P^-1 dA) = Eb known
	exactly (P = s^2 I + F F^T): the regression estimator mean(a) + beta (Eb - mean(b)), beta = cov(a, b) / var(b) from the samples (0 with fewer
	than 4 samples or a constant b); standard error = the residual standard deviation (two fitted constants) / sqrt(t).  Where the
	preconditioner is exact a_c = b_c and the random part vanishes, as it does in the value; where it is weak beta -> 0."""
	t = len(a)
	vb = float(np.var(b, ddof=1)) if t >= 4 else 0.0
	beta = float(np.cov(a, b)[0, 1] / vb) if vb > 0 else 0.0
	res = a - beta * b
	return float(a.mean() + beta * (Eb - b.mean())), float(np.std(res, ddof=2 if beta != 0.0 else 1) / np.sqrt(t))


class _EstimateFn(torch.autograd.Function):
	"""Autograd node of IterativeGaussianProcess.log_marginal_estimate: value and gradient estimates come from the same solve."""

	@staticmethod
	def forward(ctx, gp, term, weight, probes, params, *tensors):
		val, grads = gp._estimate(term, weight, probes, params)
		ctx.grads = grads
		return val.clone()

	@staticmethod
	def backward(ctx, gout):
		scale = gout.reshape(-1)[0]
		return (None, None, None, None, None) + tuple(scale.to(g.device) * g for g in ctx.grads)


class _EstimateView(IterativeGaussianProcess):
	"""The estimator as Estimator.optimize_params_general sees it inside optimize_params_estimate: its ``log_marginal`` is the estimate.  Shares
	the state of the object it views (same __dict__); the public class goes on refusing ``log_marginal``."""

	def log_marginal(self, kernel, X, weight):
		return self.log_marginal_estimate(kernel, X, weight)
