"""
LocalExpertsGaussianProcess: a committee of exact local GP experts (Deisenroth and Ng, "Distributed Gaussian Processes", ICML 2015) behind the
estimator surface of ``GaussianProcess``.  The reference has no counterpart, as ``IterativeGaussianProcess`` has none; this is the third scale
regime of the package:

    dense factorisation (GaussianProcess)        exact, N <= 131 072 on one GPU
    matrix-free (IterativeGaussianProcess)       exact, any N, a block solve per 64 test points, a randomised evidence
    local experts (this class)                   an APPROXIMATION: E = ceil(N / expert_size) independent exact GPs on blocks of at most 512
                                                 points, trained on the factorised evidence sum_e lml_e with its exact gradient, combined
                                                 by PoE / gPoE / BCM / rBCM -- a million points, predictions in milliseconds

What runs where
  per-expert Gram fill, Cholesky, L^-T, alpha, evidence, gradient     stpy_experts_fit      (csrc/experts.hip; one workgroup per expert)
  per-expert mean and latent variance at the test points              stpy_experts_predict  (one workgroup per expert and 32 test points)
  combination over experts                                            stpy_experts_combine  (one thread per test point)
  the same two with input gradients (mean_std_grad, ucb_optimize):
    per-expert mean, variance and their gradients, w = K_e^-1 k*      stpy_experts_predict_grad  (same grid; two triangular MFMA products)
    combination and its chain rule (clamp, rBCM's weights)            stpy_experts_combine_grad  (one thread per test point)
  routed prediction (``predict_experts=k``):
    every expert's centroid in scaled coordinates, once per fit       stpy_experts_centroids     (one wave per expert)
    the k nearest experts of every test point                         stpy_experts_route         (one wave per test point)
    the selected experts' predictions (and gradients), k slots        stpy_experts_predict_routed(_grad)  (one workgroup per tile of a work list)
    combination over the k slots                                      stpy_experts_combine(_grad), unchanged, with E := k
Python partitions (numpy on the host; "kdtree": torch sorts and segment reductions on the device, level by level), gathers the points by expert
(one device index_select), builds the routed work lists (device integer operations, no read-back), sequences those launches and owns the tensors.

Spatial partition and routing.  ``partition="kdtree"`` cuts the data into the balanced sizes of "random" as the leaves of a k-d tree over the
kernel's scaled coordinates x[:, cols] / lengthscale (the rule: ``kdtree_order``), taken with the lengthscales current at ``fit_gp``;
``log_marginal`` and ``optimize_params`` work on the current partition and the refit at the end of ``optimize_params`` repartitions.  With
``predict_experts=k`` every prediction (``mean_std`` / ``mean_var`` / ``mean`` / ``ucb`` / ``lcb``, ``mean_std_grad``, ``ucb_optimize``) asks only
the k experts whose centroids are nearest to the test point (``route``): k M (expert, point) pairs in place of E M, whatever N is; a value above E
means all experts, a value above the routing kernel's cap of 16 with more than 16 experts is refused.  The combination then runs over the k
slots: gPoE's beta is 1 / k and BCM's correction (1 - k) / kappa.  Three launches per chunk (route, routed prediction, combination) in place of
two; a fit makes one more (the centroids).  ``expert_mean_var`` / ``expert_mean_var_grad`` stay all-experts diagnostics.  Routing works with
every partition but is ACCURATE only on a spatial one: under rBCM a far expert returns var_e ~ kappa and weighs ~ 0, which is what makes it
safe to skip -- and on a random partition no expert is far.  RMSE against the noiseless f = sin(6 x_0) cos(5 x_1) + 0.5 x_{d-1} on the unit
cube, 300 test points, SE kernel, rBCM (tests/test_experts_route_cpu.py, NumPy oracle):
    case                                      random, all E   random, k = 4   kdtree, all E   kdtree, k = 4
    N 2048, d 2, size 64, ls .15, s .1            .0200           .0525           .0268           .0269
    N 2048, d 3, size 64, ls .30, s .1            .0483           .0704           .0354           .0357
    N 1000, d 2, size 48, ls .15, s .05           .0207           .0358           .0205           .0206
The routed posterior is piecewise smooth: it jumps where the k-th and the (k + 1)-th nearest expert of a point swap, and ``mean_std_grad`` is
the gradient of the function computed WITH THE SELECTION HELD FIXED.

The hyper-parameters are shared by all experts; the kernel is ONE stationary term (SE / Matern 1/2, 3/2, 5/2, isotropic or ARD, on a column
group or on all columns), float64 only.  Variances are those of the latent f (no noise term), as in the dense class; like every ``mean_std`` /
``mean_var`` of the package the second return value is a standard deviation.

``mean_std_grad`` returns the input gradients of the combined mean and standard deviation -- of the function ``mean_std`` computes, clamp and
rBCM weights included -- and ``ucb_optimize`` climbs the acquisition from all its starts as one stacked L-BFGS-B problem, two launches per
evaluation and chunk.

Out of scope (refused with the reason): autograd through a test tensor with ``requires_grad`` (use ``mean_std_grad``), ``ucb_optimize`` before a
fit, spatial partitions other than "kdtree" and a user-given assignment (k-means), routing by anything but centroid distance, overlapping or
hierarchical experts, appending and deleting points, float32, an explicit ``Sigma``, composite kernels, several GPUs.
"""
import numpy as np
import torch

from .. import _lib
from ..estimator import Estimator
from ..kernels import KernelFunction
from .nystrom_fea import _check_term_overrides, _stationary_term

ROUTE_CAP = 16                       # stpy_experts_route_max_k(): checked against the library at the first fit with predict_experts
EXPERT_CAP = 512                     # stpy_experts_max_n(): checked against the library at the first fit (the constructor stays on the host)
COMBINE_MODES = {"poe": 0, "gpoe": 1, "bcm": 2, "rbcm": 3}
# test points of one predict launch: E * chunk stays at or below this many (mu_e, var_e) elements; the launch's workspace is 8 * 32 * ceil(chunk / 32)
# * E * (largest expert rounded up to 32) bytes -- 2 GiB at experts of 256 points, 4 GiB at 512
PREDICT_BUDGET = 1 << 20


def balanced_sizes(n, expert_size):
	"""Sizes of E = ceil(n / expert_size) pieces of n points that differ by at most one, the larger ones first."""
	n, expert_size = int(n), int(expert_size)
	if n <= 0:
		return np.zeros((0,), dtype=np.int64)
	E = -(-n // expert_size)
	base, extra = divmod(n, E)
	return np.asarray([base + 1] * extra + [base] * (E - extra), dtype=np.int64)


def kdtree_order(z, sizes):
	"""The k-d partition of the points z (n, d) -- scaled coordinates x[:, cols] * inv_ls, a tensor on any device -- into len(sizes) leaves of the
	given sizes, left to right; returns the point indices leaf by leaf (int64, on z's device), ascending within a leaf.  A node owns the leaves
	[a, b) and a set of points: with b - a == 1 it is that leaf; otherwise mid = a + ceil((b - a) / 2), the split coordinate is the one with the
	largest max z - min z over the node's points (ties: the lowest position), the points are sorted by (z in that coordinate, original index), the
	first sum(sizes[a:mid]) go left and the rest right.  Run level by level, ceil(log2 E) of them, every node of a level at once: per level a
	segment max / min (scatter_reduce), two stable sorts and a gather on the device, and O(E) index arithmetic on the host."""
	sizes = np.asarray(sizes, dtype=np.int64)
	n, d, dev = int(z.shape[0]), int(z.shape[1]), z.device
	csum = np.concatenate([[0], np.cumsum(sizes)])
	a, b = np.zeros(1, dtype=np.int64), np.full(1, len(sizes), dtype=np.int64)
	node = torch.zeros((n,), dtype=torch.int64, device=dev)          # the node of every point, in the order of the data
	iota, pos_d = torch.arange(n, dtype=torch.int64, device=dev), torch.arange(d, dtype=torch.int64, device=dev)
	while n and np.any(b - a > 1):
		nn = len(a)
		split = b - a > 1
		mid = np.where(split, a + (b - a + 1) // 2, b)
		left = torch.from_numpy(csum[mid] - csum[a]).to(dev)                    # points that stay left (a leaf keeps all of its points)
		first = np.concatenate([[0], np.cumsum(1 + split.astype(np.int64))])[:-1]          # the left child's number on the next level
		idx = node.unsqueeze(1).expand(n, d).contiguous()
		hi = torch.full((nn, d), -float("inf"), dtype=z.dtype, device=dev).scatter_reduce_(0, idx, z, "amax", include_self=True)
		lo = torch.full((nn, d), float("inf"), dtype=z.dtype, device=dev).scatter_reduce_(0, idx, z, "amin", include_self=True)
		spread = hi - lo
		coord = torch.where(spread == spread.max(dim=1, keepdim=True).values, pos_d, d).min(dim=1).values.clamp_(max=d - 1)
		key = z.gather(1, coord[node].unsqueeze(1)).squeeze(1)
		o1 = torch.argsort(key, stable=True)                                    # by (key, original index) ...
		order = o1[torch.argsort(node[o1], stable=True)]                       # ... within every node
		ns = node[order]
		start = torch.from_numpy(csum[a]).to(dev)
		right = (iota - start[ns]) >= left[ns]
		node = torch.empty_like(node).scatter_(0, order, torch.from_numpy(first).to(dev)[ns] + right.long())
		na, nb = np.empty(nn + int(split.sum()), dtype=np.int64), np.empty(nn + int(split.sum()), dtype=np.int64)
		na[first], nb[first] = a, mid
		na[first[split] + 1], nb[first[split] + 1] = mid[split], b[split]
		a, b = na, nb
	return torch.argsort(node, stable=True)


def partition_points(n, expert_size, partition="random", seed=0, z=None):
	"""(order, sizes): ``order`` lists the point indices expert by expert, ``sizes[e]`` is the number of points of expert e.  "random": a
	numpy.random.default_rng(seed) permutation cut into balanced pieces; "contiguous": the given order cut the same way; "kdtree": the same
	sizes, left to right, as the leaves of a k-d tree over the scaled coordinates ``z`` (n, d) (``kdtree_order``); an integer array / tensor of
	n expert ids: the points of expert e in their given order, E = largest id + 1."""
	n = int(n)
	if isinstance(partition, str):
		if partition not in ("random", "contiguous", "kdtree"):
			raise ValueError("LocalExpertsGaussianProcess: partition=%r (\"random\", \"contiguous\", \"kdtree\" or an integer tensor of expert ids)" % (partition,))
		sizes = balanced_sizes(n, expert_size)
		if partition == "kdtree" and n > 0:
			if z is None or int(z.shape[0]) != n:
				raise ValueError("LocalExpertsGaussianProcess: partition=\"kdtree\" needs the scaled coordinates z of the n points")
			return kdtree_order(z, sizes).cpu().numpy().astype(np.int64), sizes
		order = np.random.default_rng(int(seed)).permutation(n) if partition == "random" else np.arange(n)
		return order.astype(np.int64), sizes
	ids = partition.detach().cpu().numpy() if torch.is_tensor(partition) else np.asarray(partition)
	if ids.dtype.kind not in "iu":
		raise ValueError("LocalExpertsGaussianProcess: an explicit partition must be an INTEGER tensor of expert ids, got %s" % ids.dtype)
	ids = ids.reshape(-1).astype(np.int64)
	if ids.shape[0] != n:
		raise ValueError("LocalExpertsGaussianProcess: the partition assigns %d points, the data has %d" % (ids.shape[0], n))
	if n and ids.min() < 0:
		raise ValueError("LocalExpertsGaussianProcess: negative expert id %d" % int(ids.min()))
	sizes = np.bincount(ids).astype(np.int64) if n else np.zeros((0,), dtype=np.int64)
	return np.argsort(ids, kind="stable").astype(np.int64), sizes


class _ExpertsEvidenceFn(torch.autograd.Function):
	"""Autograd node of LocalExpertsGaussianProcess.log_marginal: ONE stpy_experts_fit launch with a gradient; backward hands out its totals."""

	@staticmethod
	def forward(ctx, gp, term, weight, params, *tensors):
		val, ctx.grads = gp._evidence(term, weight, params)
		return val.clone()

	@staticmethod
	def backward(ctx, gout):
		scale = gout.reshape(-1)[0]
		return (None, None, None, None) + tuple(scale.to(g.device) * g for g in ctx.grads)


class LocalExpertsGaussianProcess(Estimator):

	def __init__(self, gamma=1, s=0.001, kappa=1., kernel_name="squared_exponential", d=1, kernel=None, nu=1.5, expert_size=256,
				 partition="random", partition_seed=0, combine="rbcm", max_size=10000, predict_experts=None, bounds=None):
		self.s = s
		self.d = d
		self.bounds = bounds                             # box of ucb_optimize: a (low, high) per coordinate
		self.optimize_info = None
		self.x = self.y = None
		self.n = 0
		self.fitted = False
		self.back_prop = True
		if kernel is not None:
			self.kernel_object = kernel
			self.d = kernel.d
		else:
			self.kernel_object = KernelFunction(kernel_name=kernel_name, gamma=gamma, nu=nu, kappa=kappa, d=d)
		self.kernel = self.kernel_object.kernel
		self.expert_size, self.partition, self.partition_seed = int(expert_size), partition, int(partition_seed)
		self.combine, self.max_size = combine, int(max_size)
		self.predict_experts = predict_experts           # None: every expert predicts everywhere; k: a test point asks its k nearest experts
		self.assignment_ = self.offsets_ = None          # host arrays: expert id of every point (given order), row range of every expert (gathered order)
		# kernel launches of this object so far: a fit is 2 and a prediction chunk is 2; with predict_experts a fit is 3 (the centroids) and a
		# chunk is 3 (route, routed prediction, combination)
		self.launches = 0
		self.lml_batch_path = "device"
		self._sizes, self._order = np.zeros((0,), dtype=np.int64), None
		self._xs = self._ys = self._offsets = self._factor = self._alpha = self._info = self._hyper = None
		self._cent, self._k = None, 0                    # the experts' centroids in scaled coordinates and min(predict_experts, E), set by a fit
		self._check()

	# ------------------------------------------------------------------ host checks
	def _check(self):
		"""Everything that can be refused without the data is refused here, on the host."""
		try:
			_stationary_term(self.kernel_object)
		except NotImplementedError as e:
			raise NotImplementedError("LocalExpertsGaussianProcess: every expert runs ONE stationary kernel term (SE / Matern / ARD) in one workgroup; "
									  "composite kernels are not supported (%s)" % e)
		if not 1 <= self.expert_size <= EXPERT_CAP:
			raise ValueError("LocalExpertsGaussianProcess: expert_size=%d outside [1, %d] (stpy_experts_max_n: an expert is factorised by one workgroup)"
							 % (self.expert_size, EXPERT_CAP))
		if self.combine not in COMBINE_MODES:
			raise ValueError("LocalExpertsGaussianProcess: combine=%r, one of %s" % (self.combine, ", ".join(repr(k) for k in COMBINE_MODES)))
		if isinstance(self.partition, str) and self.partition not in ("random", "contiguous", "kdtree"):
			raise ValueError("LocalExpertsGaussianProcess: partition=%r (\"random\", \"contiguous\", \"kdtree\" or an integer tensor of expert ids)" % (self.partition,))
		k = self.predict_experts
		if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1):
			raise ValueError("LocalExpertsGaussianProcess: predict_experts=%r (None: all experts, or the number k >= 1 of nearest experts a test point asks)" % (k,))
		if self.max_size < 1:
			raise ValueError("LocalExpertsGaussianProcess: max_size must be positive")

	@staticmethod
	def _no_grad(xtest):
		if torch.is_tensor(xtest) and xtest.requires_grad:
			raise NotImplementedError("LocalExpertsGaussianProcess: no autograd through the test tensor (requires_grad); the input gradients of the "
									  "combined posterior are what mean_std_grad returns -- pass a test tensor without requires_grad")

	def description(self):
		return self.kernel_object.description() + "\nlambda=" + str(self.s) + "\nlocal experts (%s, expert_size %d, %d experts, partition %s)" % (
			self.combine, self.expert_size, len(self._sizes), self.partition if isinstance(self.partition, str) else "given")

	@property
	def experts_info(self):
		"""E, the experts' sizes, the kernel launches so far and the bytes of the resident factor buffer (host bookkeeping only).  An object that
		opted into the k-d partition or into routing also reports "partition" (its name; "given" for an id array) and "predict_experts" (as
		given; the number in use is min(predict_experts, E))."""
		E = int(len(self._sizes))
		npm = -(-int(self._sizes.max()) // 32) * 32 if E else 0
		info = {"E": E, "sizes": [int(v) for v in self._sizes], "launches": int(self.launches), "factor_bytes": 8 * E * npm * npm if self.fitted else 0}
		if self.predict_experts is not None or (isinstance(self.partition, str) and self.partition == "kdtree"):
			info.update(partition=self.partition if isinstance(self.partition, str) else "given",
						predict_experts=None if self.predict_experts is None else int(self.predict_experts))
		return info

	def add_data_point(self, *args, **kwargs):
		raise NotImplementedError("LocalExpertsGaussianProcess.add_data_point: appending to a fitted committee is not implemented; refit")

	def remove_data_point(self, *args, **kwargs):
		raise NotImplementedError("LocalExpertsGaussianProcess.remove_data_point: deleting from a fitted committee is not implemented; refit")

	# ------------------------------------------------------------------ fit
	def fit(self, x=None, y=None):
		if x is not None:
			self.fit_gp(x, y)
		else:
			self.fit_gp(self.x, self.y)

	def _check_data(self, x, Sigma=None):
		if Sigma is not None:
			raise NotImplementedError("LocalExpertsGaussianProcess: an explicit Sigma couples the experts; the noise is s^2 I")
		dt = x.dtype if torch.is_tensor(x) else np.asarray(x).dtype
		if dt in (torch.float32, np.dtype("float32")):
			raise NotImplementedError("LocalExpertsGaussianProcess: float32 data; the expert kernels are float64 only (a 512-point Cholesky in "
									  "one workgroup has no fp32 route)")

	def _partition(self, n, x=None):
		z = None
		if isinstance(self.partition, str) and self.partition == "kdtree" and n:
			# scaled coordinates under the lengthscales current now, on the device where the data are: one multiplication per entry
			xd = _lib.to_device(x, torch.float64)
			term = _stationary_term(self.kernel_object)
			cols, inv_ls = self.kernel_object._term_operands(term, xd, xd.dtype, xd.device)
			z = (xd if cols is None else xd.index_select(1, cols.long())) * inv_ls
		order, sizes = partition_points(n, self.expert_size, self.partition, self.partition_seed, z=z)
		over = np.nonzero(sizes > EXPERT_CAP)[0]
		if over.size:
			raise ValueError("LocalExpertsGaussianProcess: expert %d has %d points, above the cap of %d (stpy_experts_max_n)"
							 % (int(over[0]), int(sizes[over[0]]), EXPERT_CAP))
		return order, sizes

	def fit_gp(self, x, y, Sigma=None):
		self._check()
		self._check_data(x, Sigma)
		n = int(x.shape[0])
		order, sizes = self._partition(n, x)       # (host, but "kdtree"; an oversized expert is refused before anything reaches the device)
		k = self.predict_experts
		if k is not None and k > ROUTE_CAP and len(sizes) > ROUTE_CAP:
			raise ValueError("LocalExpertsGaussianProcess: predict_experts=%d with %d experts: the routing kernel selects at most %d "
							 "(stpy_experts_route_max_k; a value above the number of experts means all of them)" % (k, len(sizes), ROUTE_CAP))
		self.n, self.d = x.shape
		self.x, self.y = x, y
		self.fitted = False
		self._factor = self._alpha = self._info = self._cent = None
		offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
		assignment = np.empty(n, dtype=np.int64)
		assignment[order] = np.repeat(np.arange(len(sizes)), sizes)
		self.assignment_, self.offsets_, self._sizes, self._order = assignment, offsets, sizes, order
		if _lib.experts_max_n() < EXPERT_CAP:
			raise _lib.StpyHipError("libstpy_hip.so accepts experts of %d points, the package expects %d" % (_lib.experts_max_n(), EXPERT_CAP))
		xd = _lib.to_device(x, torch.float64)
		yd = _lib.to_device(y, torch.float64).reshape(-1)
		idx = torch.from_numpy(order).to(xd.device)
		self._xs, self._ys = xd.index_select(0, idx).contiguous(), yd.index_select(0, idx).contiguous()
		self._offsets = torch.from_numpy(offsets.astype(np.int32)).to(xd.device)
		if n == 0:
			return None
		term = _stationary_term(self.kernel_object)
		nmax, E = int(sizes.max()), len(sizes)
		factor = _lib.experts_factor(nmax, E, xd)
		alpha = torch.empty((n,), dtype=torch.float64, device=xd.device)
		cols, inv_ls, noise = self._operands(term, float(self.s))
		_, _, _, info, packed = _lib.experts_fit(term['kind'], self._xs, self._ys, self._offsets, nmax, inv_ls, noise, term['kappa'], 1.0, factor, alpha, cols=cols)
		self.launches += 2
		self._raise_failed(packed.cpu().numpy()[-4 * E:].view(np.int32), "fit_gp")          # the one read-back of a fit (waits for the launch)
		self._factor, self._alpha, self._info = factor, alpha, info
		self._hyper = (term['kind'], float(term['kappa']), cols, inv_ls, nmax)
		if self.predict_experts is not None:          # the centroids, once per fit
			if _lib.experts_route_max_k() < ROUTE_CAP:
				raise _lib.StpyHipError("libstpy_hip.so routes to %d experts, the package expects %d" % (_lib.experts_route_max_k(), ROUTE_CAP))
			self._k = min(int(self.predict_experts), E)
			self._cent = _lib.experts_centroids(self._xs, self._offsets, inv_ls, cols=cols)
			self.launches += 1
		self.fitted = True
		return None

	def _operands(self, term, s):
		xs = self._xs
		cols, inv_ls = self.kernel_object._term_operands(term, xs, xs.dtype, xs.device)
		return cols, inv_ls, torch.tensor([float(s)], dtype=torch.float64).to(xs.device)

	@staticmethod
	def _raise_failed(info, what):
		bad = np.nonzero(info)[0]
		if bad.size:
			e, piv = int(bad[0]), int(info[bad[0]])
			if piv < 0:
				raise _lib.StpyHipError("LocalExpertsGaussianProcess.%s: expert %d does not fit the sizes the launch was made for (info %d)" % (what, e, piv))
			raise torch.linalg.LinAlgError("LocalExpertsGaussianProcess.%s: expert %d: the leading minor of order %d of K_e + s^2 I is not positive definite "
										   "(%d of %d experts failed)" % (what, e, piv, int(bad.size), int(info.shape[0])))

	@property
	def A(self):
		"""The experts' K_e^-1 y_e, in the order of the data, (N, 1)."""
		if self._alpha is None:
			return None
		out = torch.empty_like(self._alpha)
		out[torch.from_numpy(self._order).to(out.device)] = self._alpha
		return _lib.like_input(out.reshape(-1, 1), self.x)

	# ------------------------------------------------------------------ prediction
	def _prior(self, xtest):
		term = _stationary_term(self.kernel_object)
		m = int(xtest.shape[0])
		dt = xtest.dtype if torch.is_tensor(xtest) and xtest.dtype.is_floating_point else torch.float64
		dev = xtest.device if torch.is_tensor(xtest) else "cpu"
		return torch.zeros((m, 1), dtype=dt, device=dev), torch.full((m, 1), float(np.sqrt(term['kappa'])), dtype=dt, device=dev)

	def _chunks(self, m):
		E = max(len(self._sizes), 1)
		step = max(1, min(self.max_size, PREDICT_BUDGET // E))
		return [(a, min(a + step, m)) for a in range(0, m, step)]

	def _experts_device(self, xt):
		"""(mu_e, var_e), (E, M) device tensors: one stpy_experts_predict launch per chunk of test points."""
		kind, kappa, cols, inv_ls, nmax = self._hyper
		E, m = len(self._sizes), xt.shape[0]
		mu_e = torch.empty((E, m), dtype=torch.float64, device=xt.device)
		var_e = torch.empty((E, m), dtype=torch.float64, device=xt.device)
		for a, b in self._chunks(m):
			_lib.experts_predict(kind, self._xs, self._offsets, nmax, inv_ls, kappa, self._factor, self._alpha, self._info, xt[a:b], mu_e[:, a:b], var_e[:, a:b], cols=cols)
			self.launches += 1
		return mu_e, var_e

	def expert_mean_var(self, xtest):
		"""Every expert's posterior mean and latent VARIANCE at the test points, two (E, M) tensors placed like ``xtest`` (diagnostics)."""
		self._no_grad(xtest)
		if not self.fitted:
			raise AttributeError("LocalExpertsGaussianProcess.expert_mean_var needs a fitted object: call fit_gp first")
		mu_e, var_e = self._experts_device(_lib.to_device(xtest, torch.float64))
		return _lib.like_input(mu_e, xtest), _lib.like_input(var_e, xtest)

	# ------------------------------------------------------------------ routing
	def _routed_chunks(self, m, per_pair=1):
		"""The routed paths' rule: k * chunk * per_pair output elements stay at or below PREDICT_BUDGET (per_pair = 1 for a prediction's pairs,
		2 + 2 d with gradients); a chunk's work list has at most chunk k / 32 + min(E, chunk k) tiles of 8 * 32 * (largest expert rounded up
		to 32) bytes of workspace each, twice that with gradients."""
		step = max(1, min(self.max_size, PREDICT_BUDGET // (self._k * per_pair)))
		return [(a, min(a + step, m)) for a in range(0, m, step)]

	def _route_device(self, xt):
		"""sel (M, k) int32 on the device: one stpy_experts_route launch."""
		kind, kappa, cols, inv_ls, nmax = self._hyper
		sel = _lib.experts_route(self._cent, inv_ls, xt, self._k, cols=cols)
		self.launches += 1
		return sel

	def route(self, xtest):
		"""The experts a routed prediction asks: an (M, k) integer tensor of expert ids, k = min(predict_experts, E), ascending in every row,
		placed like ``xtest`` -- the k experts whose centroids (means of their points in the kernel's scaled coordinates) are nearest to the
		test point, ties going to the lower id, experts without points last.  One launch per chunk of ``max_size`` points."""
		self._no_grad(xtest)
		if self.predict_experts is None:
			raise ValueError("LocalExpertsGaussianProcess.route: the object was made with predict_experts=None (every expert predicts everywhere)")
		if not self.fitted:
			raise AttributeError("LocalExpertsGaussianProcess.route needs a fitted object: call fit_gp first")
		xt = _lib.to_device(xtest, torch.float64)
		m = xt.shape[0]
		sel = torch.empty((m, self._k), dtype=torch.int32, device=xt.device)
		for a, b in self._routed_chunks(m):
			sel[a:b] = self._route_device(xt[a:b])
		return _lib.like_input(sel.long(), xtest)

	def _mean_var_routed(self, xt):
		"""``_mean_var_device`` with routing: per chunk stpy_experts_route, the work list (device integer operations, no read-back),
		stpy_experts_predict_routed into (k, chunk) slots and stpy_experts_combine over the k slots: three launches."""
		kind, kappa, cols, inv_ls, nmax = self._hyper
		E, k, m, d = len(self._sizes), self._k, xt.shape[0], inv_ls.numel()
		mu = torch.empty((m,), dtype=torch.float64, device=xt.device)
		var = torch.empty((m,), dtype=torch.float64, device=xt.device)
		chunks = self._routed_chunks(m)
		work = _lib.experts_predict_routed_workspace(nmax, d, _lib.experts_route_tiles(E, max(b - a for a, b in chunks), k), xt) if chunks else None
		for a, b in chunks:
			wexp, wpair = _lib.experts_work_list(self._route_device(xt[a:b]), E)
			mu_s = torch.empty((k, b - a), dtype=torch.float64, device=xt.device)
			var_s = torch.empty((k, b - a), dtype=torch.float64, device=xt.device)
			_lib.experts_predict_routed(kind, self._xs, self._offsets, nmax, inv_ls, kappa, self._factor, self._alpha, self._info, xt[a:b], wexp, wpair,
										mu_s, var_s, cols=cols, work=work)
			_lib.experts_combine(COMBINE_MODES[self.combine], mu_s, var_s, kappa, mu[a:b], var[a:b])
			self.launches += 2
		return mu, var

	def _mean_var_grad_routed(self, xt):
		"""``_mean_var_grad_device`` with routing: per chunk stpy_experts_route, the work list, stpy_experts_predict_routed_grad and
		stpy_experts_combine_grad over the k slots: three launches.  The selection is held fixed under the derivative."""
		kind, kappa, cols, inv_ls, nmax = self._hyper
		E, k, m, d = len(self._sizes), self._k, xt.shape[0], inv_ls.numel()
		mu = torch.empty((m,), dtype=torch.float64, device=xt.device)
		var = torch.empty((m,), dtype=torch.float64, device=xt.device)
		dmu = torch.empty((m, d), dtype=torch.float64, device=xt.device)
		dstd = torch.empty((m, d), dtype=torch.float64, device=xt.device)
		chunks = self._routed_chunks(m, 2 + 2 * d)
		work = _lib.experts_predict_routed_workspace(nmax, d, _lib.experts_route_tiles(E, max(b - a for a, b in chunks), k), xt, grad=True) if chunks else None
		for a, b in chunks:
			wexp, wpair = _lib.experts_work_list(self._route_device(xt[a:b]), E)
			mu_s = torch.empty((k, b - a), dtype=torch.float64, device=xt.device)
			var_s = torch.empty((k, b - a), dtype=torch.float64, device=xt.device)
			gmu_s = torch.empty((k, b - a, d), dtype=torch.float64, device=xt.device)
			gvar_s = torch.empty((k, b - a, d), dtype=torch.float64, device=xt.device)
			_lib.experts_predict_routed_grad(kind, self._xs, self._offsets, nmax, inv_ls, kappa, self._factor, self._alpha, self._info, xt[a:b], wexp, wpair,
											 mu_s, var_s, gmu_s, gvar_s, cols=cols, work=work)
			_lib.experts_combine_grad(COMBINE_MODES[self.combine], mu_s, var_s, gmu_s, gvar_s, kappa, mu[a:b], var[a:b], dmu[a:b], dstd[a:b])
			self.launches += 2
		return mu, var, dmu, dstd

	def _mean_var_device(self, xt):
		if self._cent is not None:
			return self._mean_var_routed(xt)
		kind, kappa, cols, inv_ls, nmax = self._hyper
		E, m = len(self._sizes), xt.shape[0]
		mu = torch.empty((m,), dtype=torch.float64, device=xt.device)
		var = torch.empty((m,), dtype=torch.float64, device=xt.device)
		for a, b in self._chunks(m):
			mu_e = torch.empty((E, b - a), dtype=torch.float64, device=xt.device)
			var_e = torch.empty((E, b - a), dtype=torch.float64, device=xt.device)
			_lib.experts_predict(kind, self._xs, self._offsets, nmax, inv_ls, kappa, self._factor, self._alpha, self._info, xt[a:b], mu_e, var_e, cols=cols)
			_lib.experts_combine(COMBINE_MODES[self.combine], mu_e, var_e, kappa, mu[a:b], var[a:b])
			self.launches += 2
		return mu, var

	def mean_std(self, xtest):
		"""Combined posterior mean and standard deviation of the latent f, (M, 1) each, placed like ``xtest``; the prior before a fit."""
		self._no_grad(xtest)
		if not self.fitted:
			return self._prior(xtest)
		xt = _lib.to_device(xtest, torch.float64)
		mu, var = self._mean_var_device(xt)
		sd = torch.empty_like(var)
		if xt.shape[0] > 0:
			_lib.predict_finish(sumsq=torch.zeros_like(var), kdiag=var, scale=0.0, sigma=sd)
		return _lib.like_input(mu.reshape(-1, 1), xtest), _lib.like_input(sd.reshape(-1, 1), xtest)

	mean_var = mean_std

	def mean(self, xtest):
		return self.mean_std(xtest)[0]

	def lcb(self, xtest):
		mu, s = self.mean_std(xtest)
		return mu - 2 * s

	def ucb(self, xtest):
		mu, s = self.mean_std(xtest)
		return mu + 2 * s

	# ------------------------------------------------------------------ input gradients
	def _grad_chunks(self, m, d):
		"""The gradient path's own rule: E * chunk * (2 + 2 d) output elements (mu_e, var_e and the two (E, chunk, d) gradient arrays) stay at or
		below PREDICT_BUDGET; the launch's workspace is twice that of a prediction of the same chunk."""
		E = max(len(self._sizes), 1)
		step = max(1, min(self.max_size, PREDICT_BUDGET // (E * (2 + 2 * d))))
		return [(a, min(a + step, m)) for a in range(0, m, step)]

	@staticmethod
	def _place(compact, D, cols):
		"""Gradients over the selected coordinates (last dimension, in cols order) -> all D columns of the test points, zero where the kernel
		term does not read: one device index_copy."""
		if cols is None:
			return compact
		out = torch.zeros(tuple(compact.shape[:-1]) + (D,), dtype=compact.dtype, device=compact.device)
		return out.index_copy_(compact.dim() - 1, cols.long(), compact)

	def _experts_grad_device(self, xt):
		"""(mu_e, var_e (E, M), gmu_e, gvar_e (E, M, d) over the selected coordinates): one stpy_experts_predict_grad launch per chunk."""
		kind, kappa, cols, inv_ls, nmax = self._hyper
		E, m, d = len(self._sizes), xt.shape[0], inv_ls.numel()
		mu_e = torch.empty((E, m), dtype=torch.float64, device=xt.device)
		var_e = torch.empty((E, m), dtype=torch.float64, device=xt.device)
		gmu_e = torch.empty((E, m, d), dtype=torch.float64, device=xt.device)
		gvar_e = torch.empty((E, m, d), dtype=torch.float64, device=xt.device)
		for a, b in self._grad_chunks(m, d):
			_lib.experts_predict_grad(kind, self._xs, self._offsets, nmax, inv_ls, kappa, self._factor, self._alpha, self._info, xt[a:b],
									  mu_e[:, a:b], var_e[:, a:b], gmu_e[:, a:b], gvar_e[:, a:b], cols=cols)
			self.launches += 1
		return mu_e, var_e, gmu_e, gvar_e

	def expert_mean_var_grad(self, xtest):
		"""Every expert's posterior mean and latent VARIANCE at the test points, (E, M), and their input gradients, (E, M, D) with zeros in the
		columns the kernel term does not read; placed like ``xtest`` (diagnostics)."""
		self._no_grad(xtest)
		if not self.fitted:
			raise AttributeError("LocalExpertsGaussianProcess.expert_mean_var_grad needs a fitted object: call fit_gp first")
		xt = _lib.to_device(xtest, torch.float64)
		mu_e, var_e, gmu_e, gvar_e = self._experts_grad_device(xt)
		cols = self._hyper[2]
		return tuple(_lib.like_input(t, xtest) for t in (mu_e, var_e, self._place(gmu_e, xt.shape[1], cols), self._place(gvar_e, xt.shape[1], cols)))

	def _mean_var_grad_device(self, xt):
		"""(mu, var (M,), dmu, dstd (M, d) over the selected coordinates): per chunk one stpy_experts_predict_grad and one
		stpy_experts_combine_grad launch.  mu and var carry the bits of ``_mean_var_device``."""
		if self._cent is not None:
			return self._mean_var_grad_routed(xt)
		kind, kappa, cols, inv_ls, nmax = self._hyper
		E, m, d = len(self._sizes), xt.shape[0], inv_ls.numel()
		mu = torch.empty((m,), dtype=torch.float64, device=xt.device)
		var = torch.empty((m,), dtype=torch.float64, device=xt.device)
		dmu = torch.empty((m, d), dtype=torch.float64, device=xt.device)
		dstd = torch.empty((m, d), dtype=torch.float64, device=xt.device)
		chunks = self._grad_chunks(m, d)
		work = _lib.experts_predict_grad_workspace(nmax, d, E, max(b - a for a, b in chunks), xt) if chunks else None
		for a, b in chunks:
			mu_e = torch.empty((E, b - a), dtype=torch.float64, device=xt.device)
			var_e = torch.empty((E, b - a), dtype=torch.float64, device=xt.device)
			gmu_e = torch.empty((E, b - a, d), dtype=torch.float64, device=xt.device)
			gvar_e = torch.empty((E, b - a, d), dtype=torch.float64, device=xt.device)
			_lib.experts_predict_grad(kind, self._xs, self._offsets, nmax, inv_ls, kappa, self._factor, self._alpha, self._info, xt[a:b],
									  mu_e, var_e, gmu_e, gvar_e, cols=cols, work=work)
			_lib.experts_combine_grad(COMBINE_MODES[self.combine], mu_e, var_e, gmu_e, gvar_e, kappa, mu[a:b], var[a:b], dmu[a:b], dstd[a:b])
			self.launches += 2
		return mu, var, dmu, dstd

	def mean_std_grad(self, xtest):
		"""Batched input gradients of the combined posterior: (d mu, d std), each (M, D), placed like ``xtest`` (GaussianProcess.mean_std_grad);
		columns the kernel term does not read are zero.  The derivative of the function ``mean_std`` computes: through the combination rule, its
		variance clamp (zero where it is active) and rBCM's variance-dependent weights.  Not fitted: zeros (the prior of a stationary kernel is
		flat), without touching the device."""
		xtest = torch.as_tensor(xtest).detach()
		m = int(xtest.shape[0])
		if not self.fitted:
			dt = xtest.dtype if xtest.dtype in (torch.float32, torch.float64) else torch.float64
			D = int(xtest.shape[1]) if xtest.dim() > 1 else int(self.d)
			return torch.zeros((m, D), dtype=dt, device=xtest.device), torch.zeros((m, D), dtype=dt, device=xtest.device)
		xt = _lib.to_device(xtest, torch.float64)
		_, _, dmu, dstd = self._mean_var_grad_device(xt)
		cols = self._hyper[2]
		return _lib.like_input(self._place(dmu, xt.shape[1], cols), xtest), _lib.like_input(self._place(dstd, xt.shape[1], cols), xtest)

	def ucb_optimize(self, beta, multistart=25, lcb=False):
		"""GaussianProcess.ucb_optimize on the committee: maximise mu + sqrt(beta) sigma (mu - sqrt(beta) sigma with ``lcb``) over ``self.bounds``
		from ``multistart`` uniform starts drawn with the reference's np.random calls in its order.  All starts are ONE stacked L-BFGS-B problem
		(``_multistart_maximize`` of gauss_procc.py); every evaluation is one stpy_experts_predict_grad and one stpy_experts_combine_grad launch
		per chunk of starts (with ``predict_experts``: three -- stpy_experts_route, stpy_experts_predict_routed_grad, stpy_experts_combine_grad --
		so ``launches`` is three times ``evaluations`` where one chunk holds the starts; every evaluation routes anew, and the gradient holds
		that selection fixed).  Returns (solution (d,), value) of the best start, never below the acquisition at any drawn start.
		``self.optimize_info``: starts, start_values, evaluations, launches."""
		from .gauss_procc import _draw_starts, _multistart_maximize
		if not self.fitted:
			raise NotImplementedError("LocalExpertsGaussianProcess.ucb_optimize: the object is not fitted, and the prior of a stationary kernel is "
									  "flat: there is nothing to climb; call fit_gp first")
		if self.bounds is None:
			raise ValueError("ucb_optimize needs box bounds: set LocalExpertsGaussianProcess.bounds to a list of (low, high) per coordinate")
		multistart = int(multistart)
		if multistart < 1:
			raise ValueError("LocalExpertsGaussianProcess.ucb_optimize: multistart=%d must be at least 1" % multistart)
		bounds = tuple((float(a), float(b)) for (a, b) in self.bounds)
		if len(bounds) != self.d:
			raise ValueError("LocalExpertsGaussianProcess.ucb_optimize: %d bounds for d=%d" % (len(bounds), self.d))
		starts = _draw_starts(multistart, self.d, bounds)
		sign, sb = (-1.0 if lcb else 1.0), float(np.sqrt(beta))
		cols, launches, first = self._hyper[2], self.launches, []

		def evaluate(xt):
			mu, var, dmu, dstd = self._mean_var_grad_device(xt)
			val = mu + sign * sb * torch.sqrt(var)
			if not first:
				first.append(val.cpu().numpy())                    # the first evaluation is at the drawn starts
			return val, self._place(dmu + sign * sb * dstd, xt.shape[1], cols)

		def value(xt):          # (the final values need no gradients: the two launches of mean_std)
			mu, var = self._mean_var_device(xt)
			return mu + sign * sb * torch.sqrt(var)

		sol, vals, evals = _multistart_maximize(evaluate, starts, bounds, self._xs.device, torch.float64, final=value)
		x0, v0 = np.asarray(starts, dtype=np.float64), first[0]
		keep = v0 > vals                                                   # the line search watches the SUM: a start its climb did not improve stays
		sol[keep], vals[keep] = x0[keep], v0[keep]
		index = int(np.argmax(vals))
		self.optimize_info = {"starts": x0, "start_values": v0, "evaluations": evals, "launches": self.launches - launches}
		return (torch.from_numpy(sol[index].copy()), torch.tensor(float(vals[index]), dtype=torch.float64))

	# ------------------------------------------------------------------ the factorised evidence
	def _check_overrides(self, kernel, X):
		"""Host refusals of log_marginal; returns (X, the one stationary term the overrides resolve to)."""
		X, term = _check_term_overrides("LocalExpertsGaussianProcess.log_marginal", "the experts' kernel", self.kernel_object, kernel, X)
		if term['premap'] is not None or term['pname'] is None or term['kind'] not in (_lib.K_SE, _lib.K_MATERN12, _lib.K_MATERN32, _lib.K_MATERN52):
			raise NotImplementedError("LocalExpertsGaussianProcess.log_marginal: the %s kernel is not one stationary term" % kernel._term_name(term))
		return X, term

	def _need_data(self, what):
		if self._xs is None or self._xs.shape[0] == 0:
			raise AttributeError("LocalExpertsGaussianProcess.%s needs data and a partition: call fit_gp first" % what)

	def _launch_evidence(self, term, weight, s, n_params, scratch):
		"""One stpy_experts_fit launch with a gradient on the current partition, into factor / alpha / workspace buffers of its own (the
		resident factor stays); returns the packed device results, unread."""
		xs = self._xs
		nmax, E = int(self._sizes.max()), len(self._sizes)
		if "factor" not in scratch:
			scratch["factor"] = _lib.experts_factor(nmax, E, xs)
			scratch["alpha"] = torch.empty((xs.shape[0],), dtype=torch.float64, device=xs.device)
			scratch["work"] = _lib.experts_fit_workspace(nmax, len(term['group']), E, xs)
		cols, inv_ls, noise = self._operands(term, s)
		pidx = self.kernel_object._term_param_slots(term, xs.device)
		w = float(weight.item()) if torch.is_tensor(weight) else float(weight)
		packed = _lib.experts_fit(term['kind'], xs, self._ys, self._offsets, nmax, inv_ls, noise, term['kappa'], w, scratch["factor"], scratch["alpha"],
								  pidx=pidx, n_params=n_params, cols=cols, work=scratch["work"])[4]
		self.launches += 2
		return packed

	@staticmethod
	def _n_params(term, given):
		return max(int(np.prod(tuple(given.shape))) if given is not None and torch.is_tensor(given) and given.dim() > 0 else 1, max(term['pidx']) + 1)

	def _evidence(self, term, weight, params):
		"""(value (1, 1) placed like the data, [gradient per entry of params]) from one launch and one read-back."""
		E = len(self._sizes)
		given = next((t for (key, name, t) in params if key != "likelihood"), None)
		n_params = self._n_params(term, given)
		out = self._launch_evidence(term, weight, float(self.s), n_params, {}).cpu().numpy()
		self._raise_failed(out[-4 * E:].view(np.int32), "log_marginal")
		total = out[:(n_params + 2) * 8].view(np.float64)
		grads = []
		for (key, name, t) in params:
			if key == "likelihood":
				g = torch.full(t.shape if t.dim() > 0 else (), float(total[1 + n_params]), dtype=torch.float64)
			else:
				if term['pname'] != name:
					raise NotImplementedError("LocalExpertsGaussianProcess.log_marginal: the kernel has no '%s' lengthscale" % name)
				g = torch.from_numpy(total[1:1 + n_params].copy()).reshape(t.shape if t.dim() > 0 else ())
			grads.append(g.to(device=t.device, dtype=t.dtype))
		val = torch.full((1, 1), float(total[0]), dtype=torch.float64)
		return (val.to(self.x.device) if torch.is_tensor(self.x) and self.x.is_cuda else val), grads

	def log_marginal(self, kernel, X, weight):
		"""The factorised evidence sum_e [1/2 y_e^T (K_e + s^2 I)^-1 y_e + 1/2 weight log det(K_e + s^2 I)] on the current partition, shape (1, 1):
		the sign, shape and omitted n/2 log 2 pi constant of GaussianProcess.log_marginal.  ``X``: overrides of the single kernel item,
		{'0': {'gamma' | 'ard_gamma': tensor}}.  If a lengthscale tensor in ``X`` or ``self.s`` requires grad the result carries an autograd node
		whose backward is the exact gradient, summed over the experts in expert order on the device.  The resident factor is left untouched."""
		X, term = self._check_overrides(kernel, X)
		self._need_data("log_marginal")
		params = self._grad_params(X, ("gamma", "ard_gamma"))
		if params:
			return _ExpertsEvidenceFn.apply(self, term, weight, params, *[t for (_, _, t) in params])
		return self._evidence(term, weight, [])[0]

	def log_marginal_batch(self, kernel, Xs, weight, s=None):
		"""``log_marginal`` and its gradient for B candidates: one stpy_experts_fit launch per candidate, enqueued back to back into shared
		scratch, one read-back each at the end.  Returns what Estimator.optimize_params_general expects: (values (B,), grads), ``grads[b]`` =
		{'0': {parameter name: tensor}} plus {'likelihood': {'sigma': ...}} when ``s`` is given.  A candidate with a failed expert gets +inf and
		zero gradients, no exception."""
		self._need_data("log_marginal_batch")
		if s is not None and len(s) != len(Xs):
			raise ValueError("log_marginal_batch: %d noise levels for %d candidates" % (len(s), len(Xs)))
		E, scratch, pending = len(self._sizes), {}, []
		for b, X in enumerate(Xs):
			X, term = self._check_overrides(kernel, X)
			given = X.get('0', {}).get(term['pname']) if X else None
			given = torch.as_tensor(given) if given is not None else None
			n_params = self._n_params(term, given)
			shape = tuple(given.shape) if given is not None and given.dim() > 0 else (n_params,)
			pending.append((term, n_params, shape, self._launch_evidence(term, weight, float(self.s if s is None else s[b]), n_params, scratch)))
		values, grads = [], []
		for term, n_params, shape, packed in pending:
			out = packed.cpu().numpy()
			total = out[:(n_params + 2) * 8].view(np.float64)
			ok = not np.any(out[-4 * E:].view(np.int32)) and np.isfinite(total[0])
			values.append(float(total[0]) if ok else float("inf"))
			g = {'0': {term['pname']: (torch.from_numpy(total[1:1 + n_params].copy()) if ok else torch.zeros(n_params, dtype=torch.float64)).reshape(shape)}}
			if s is not None:
				g['likelihood'] = {'sigma': torch.tensor([float(total[1 + n_params]) if ok else 0.0], dtype=torch.float64)}
			grads.append(g)
		self.lml_batch_path = "device"
		values = torch.tensor(values, dtype=torch.float64)
		return (values.to(self.x.device) if torch.is_tensor(self.x) and self.x.is_cuda else values), grads

	def optimize_params(self, type='bandwidth', restarts=10, regularizer=None, maxiter=1000, mingradnorm=1e-4, verbose=False, optimizer="pymanopt",
						scale=1., weight=1., save=False, save_name='model.np', init_func=None, bounds=None, parallel=False, cores=None):
		"""GaussianProcess.optimize_params for ``type`` in {"bandwidth", "bandwidth+noise"} with the factorised evidence for the objective: the
		same parameter dictionary through Estimator.optimize_params_general, which writes the best point back and refits."""
		if type not in ("bandwidth", "bandwidth+noise"):
			raise NotImplementedError("LocalExpertsGaussianProcess.optimize_params(type='%s'): 'bandwidth' and 'bandwidth+noise' only" % type)
		if regularizer is not None:
			raise NotImplementedError("LocalExpertsGaussianProcess.optimize_params: no regularizer")
		self._need_data("optimize_params")
		params = self._bandwidth_params(type, init_func, bounds)
		return self.optimize_params_general(params=params, restarts=restarts, optimizer=optimizer, maxiter=maxiter, mingradnorm=mingradnorm,
											verbose=verbose, scale=scale, weight=weight, save=save, save_name=save_name, parallel=parallel, cores=cores)
