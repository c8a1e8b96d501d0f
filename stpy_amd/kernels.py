"""
Drop-in for ``stpy.kernels.KernelFunction`` on the Gram-matrix hot path (reference:
stpy/kernels.py:10-261 dispatcher, :136-159 ``kernel``, :368-398 SE, :552-583 ARD,
:811-859 Matern, :917-970 ARD-Matern, :300-320 linear, :620-725 additive-group SE/ARD,
:464-549 full-covariance SE / Matern, :744-761 polynomial).

Same constructor arguments, same ``kernel(a, b, **kwargs) -> (|b|, |a|)`` orientation, same ``+`` /
``*`` algebra and the same kwargs-override protocol (``kernel(a, b, **{'0': {'gamma': g}})``) that
``Estimator.optimize_params_general`` uses to talk to a kernel (estimator.py:156-171).  The
arithmetic runs in ``stpy_gram`` (stpy_amd/csrc/gram.hip); there is no CPU path.
"""
import math
from collections import OrderedDict

import torch

from . import _lib

# kernel families implemented on the device; everything else in kernels.py:167-261 is outside
# the hot path and raises.
_SUPPORTED = ("squared_exponential", "ard", "matern", "ard_matern", "linear", "ard with groups", "squared_exponential_per_group",
			  "ard_per_group", "full_covariance_se", "full_covariance_matern", "polynomial")
_OUT_OF_SCOPE = ("laplace", "modified_matern", "custom", "tanh", "step", "angsim", "gibbs", "gibbs_custom", "random_map")

_MATERN_KIND = {0.5: _lib.K_MATERN12, 1.5: _lib.K_MATERN32, 2.5: _lib.K_MATERN52}

_const_cache = OrderedDict()
_CONST_CACHE_ENTRIES = 4096


def _scalar(v):
	"""gamma / kappa may arrive as python numbers or 0-d / 1-element tensors (estimator.py:160-166)."""
	if torch.is_tensor(v):
		return float(v.detach().reshape(-1)[0].item())
	return float(v)


def _dev_const(values, dtype, device, int32=False):
	"""Small constant device arrays (inverse lengthscales, column indices), cached by value.
	Least-recently-used entries are dropped one at a time (a hyper-parameter search creates a new lengthscale key on
	every evaluation); an entry used from a stream other than the one it was allocated on is recorded on that stream,
	so the caching allocator does not hand its block out again while kernels queued there may still read it."""
	key = (tuple(values), dtype if not int32 else "i32", device.index)
	cur = torch.cuda.current_stream(device)
	ent = _const_cache.get(key)
	if ent is None:
		while len(_const_cache) >= _CONST_CACHE_ENTRIES:
			_const_cache.popitem(last=False)
		t = torch.tensor(list(values), dtype=torch.int32 if int32 else dtype, device=device)
		ent = (t, {cur.cuda_stream})
		_const_cache[key] = ent
	else:
		_const_cache.move_to_end(key)
		if cur.cuda_stream not in ent[1]:
			ent[0].record_stream(cur)
			ent[1].add(cur.cuda_stream)
	return ent[0]


class KernelFunction:

	def __init__(self, kernel_function=None, kernel_name="squared_exponential",
				 freq=None, groups=None, d=1, gamma=1, ard_gamma=None, nu=1.5, kappa=1, map=None, power=2,
				 cov=None, params=None, group=None, offset=0.):
		if kernel_function is not None:
			raise NotImplementedError("custom python kernel functions are outside the stpy_amd hot path")
		self.offset = offset
		self.optkernel = kernel_name
		self.gamma = gamma
		if ard_gamma is None:
			self.ard_gamma = torch.ones(d).double()
		else:
			# kernels.py:36-39: Tensor([ard_gamma]) if that works, else keep as given
			try:
				self.ard_gamma = torch.Tensor([ard_gamma]).double()
			except Exception:
				self.ard_gamma = ard_gamma
		self.power = power
		self.v = nu
		if params is not None:
			self.initial_params = params
		else:
			self.initial_params = {'kappa': kappa}
		self.cov = torch.eye(d).double() if cov is None else cov
		self.group = [i for i in range(d)] if group is None else group
		self.map = map
		self.groups = groups
		self.kappa = kappa
		self.freq = freq
		self.d = d
		self.add = False

		self.params = self._initial_item_params()
		# one entry per kernel item: the KernelFunction object whose attributes are the fallbacks
		# for parameters missing from an override dict (bound-method semantics of kernels.py:68)
		self._owners = [self]
		self.optkernel_list = [self.optkernel]
		self.params_dict = {'0': self.params}
		self.kernel_items = 1
		self.operations = ["-"]

	# ------------------------------------------------------------------ construction helpers
	def _initial_item_params(self):
		"""kernels.py:167-261 (get_kernel_internal): the stored parameter dictionary of one item."""
		params = {**self.initial_params, 'kappa': self.kappa, 'group': self.group, 'offset': self.offset}
		name = self.optkernel
		if name == "squared_exponential":
			params = dict(**params, **{'gamma': self.gamma})
		elif name == "ard" and self.groups is None:
			params = dict(**params, **{'ard_gamma': self.ard_gamma})
		elif name == "linear":
			pass
		elif name == "matern":
			params = dict(**params, **{'gamma': self.gamma, 'nu': self.v})
		elif name == "ard_matern":
			params = dict(**params, **{'ard_gamma': self.ard_gamma, 'nu': self.v})
		elif name == "full_covariance_se":
			params = dict(**params, **{'cov': self.cov})
		elif name == "full_covariance_matern":
			params = dict(**params, **{'cov': self.cov, 'nu': self.v})
		elif name == "polynomial" and self.groups is None:
			params = dict(**params, **{'degree': self.power})
		elif name == "polynomial":
			# kernels.py:763-788 subsets the columns of an already subset matrix with `group` again and
			# raises for any proper grouping (pinned by tests/golden K2 'poly_additive_raises')
			raise NotImplementedError("the additive polynomial kernel does not evaluate in the reference either (kernels.py:763-788)")
		elif name == "ard":
			params = dict(**params, **{'ard_gamma': self.ard_gamma, 'groups': self.groups})
		elif name in ("squared_exponential_per_group", "ard_per_group") and self.groups is not None:
			params = dict(**params, **{'groups': self.groups})
		elif name in _OUT_OF_SCOPE:
			raise NotImplementedError("kernel '%s' is outside the stpy_amd hot path (supported: %s)" % (name, ", ".join(_SUPPORTED)))
		else:
			raise AssertionError("Kernel not implemented.")     # kernels.py:261
		return params

	def __combine__(self, second_kernel_object):
		"""kernels.py:76-82."""
		self._owners = self._owners + second_kernel_object._owners
		self.optkernel_list = self.optkernel_list + second_kernel_object.optkernel_list
		self.operations = self.operations + second_kernel_object.operations[1:]
		for key, value in second_kernel_object.params_dict.items():
			self.params_dict[str(self.kernel_items)] = value
			self.kernel_items += 1

	def __add__(self, second_kernel_object):
		"""kernels.py:84-89."""
		self.__combine__(second_kernel_object)
		diff = len(set(second_kernel_object.group) - set(self.group))
		self.d += diff
		self.operations.append("+")
		return self

	def __mul__(self, second_kernel_object):
		"""kernels.py:91-94."""
		self.__combine__(second_kernel_object)
		self.operations.append("*")
		return self

	def description(self):
		"""kernels.py:96-103."""
		desc = "Kernel description:"
		for index in range(0, self.kernel_items, 1):
			desc = desc + "\n\n\tkernel: " + self.optkernel_list[index]
			desc = desc + "\n\toperation: " + self.operations[index]
			desc = desc + "\n\t" + "\n\t".join(
				["{0}={1}".format(key, value) for key, value in self.params_dict[str(index)].items()])
		return desc

	def add_groups(self, dict):
		"""kernels.py:105-110."""
		for a in self.params_dict.keys():
			if a not in dict.keys():
				dict[a] = {}
			dict[a]['group'] = self.params_dict[a]['group']
		return dict

	def get_param_refs(self):
		return self.params_dict

	def get_kernel(self):
		return self.kernel

	# ------------------------------------------------------------------ parameter resolution
	def _resolve(self, kwargs):
		"""
		kernels.py:138-157: with kwargs present they *replace* params_dict (only 'group' is
		re-injected); a key missing from an item's dict falls back to the owning object's attribute.
		Returns one launch description per kernel item.
		"""
		if len(kwargs) > 0:
			params_dict = kwargs
			self.add_groups(params_dict)
		else:
			params_dict = self.params_dict
		items = []
		for i in range(self.kernel_items):
			owner = self._owners[i]
			arg = params_dict[str(i)] if str(i) in params_dict.keys() else {}
			name = self.optkernel_list[i]
			kappa = _scalar(arg['kappa']) if 'kappa' in arg else _scalar(owner.kappa)
			group = list(arg['group']) if 'group' in arg else list(owner.group)

			def term(kind, inv_ls, cols=None, k=None, offset=0.0, premap=None, pname=None, pidx=None):
				# pname / pidx: which hyper-parameter ('gamma' / 'ard_gamma') and which of its entries sets the
				# lengthscale of each coordinate -- what the evidence gradient scatters into
				return dict(kind=kind, kappa=kappa if k is None else k, group=group if cols is None else list(cols), inv_ls=inv_ls,
							offset=offset, premap=premap, pname=pname, pidx=pidx)

			def vec(v):
				return torch.as_tensor(v).detach().double().reshape(-1)

			if name == "squared_exponential":
				gamma = _scalar(arg['gamma']) if 'gamma' in arg else _scalar(owner.gamma)
				terms = [term(_lib.K_SE, [1.0 / gamma] * len(group), pname='gamma', pidx=[0] * len(group))]
			elif name == "ard" and ('groups' in arg or owner.groups is not None):
				# kernels.py:697-725: columns subset by `group`, every entry of `groups` then indexes that
				# subset and ard_gamma; each term carries kappa, the mean is over the groups
				g = vec(arg['ard_gamma'] if 'ard_gamma' in arg else owner.ard_gamma)
				groups = arg['groups'] if 'groups' in arg else owner.groups
				terms = [term(_lib.K_SE, [1.0 / float(g[j]) for j in ga], cols=[group[j] for j in ga], k=kappa / len(groups),
							  pname='ard_gamma', pidx=list(ga)) for ga in groups]
			elif name == "ard":
				g = vec(arg['ard_gamma'] if 'ard_gamma' in arg else owner.ard_gamma)
				terms = [term(_lib.K_SE, [1.0 / float(g[j]) for j in group], pname='ard_gamma', pidx=list(group))]   # kernels.py:572
			elif name == "squared_exponential_per_group":
				# kernels.py:669-695: kappa * mean_g SE_g, and SE_g applies kappa again (the overriding one
				# if present, else the object's)
				if 'gamma_per_group' not in arg:
					raise AssertionError("This kernel requires 'gamma_per_group' initial parameters")
				groups = arg['groups'] if 'groups' in arg else owner.groups
				gpg = [_scalar(v) for v in arg['gamma_per_group']]
				terms = [term(_lib.K_SE, [1.0 / gam] * len(ga), cols=ga, k=kappa * kappa / len(groups)) for ga, gam in zip(groups, gpg)]
			elif name == "ard_per_group":
				# kernels.py:620-667: consecutive slices of the lengthscale vector belong to consecutive groups
				if 'ard_per_group' not in arg:
					raise AssertionError("This kernel requires 'ard_per_group' initial parameters")
				groups = arg['groups'] if 'groups' in arg else owner.groups
				g = vec(arg['ard_per_group'])
				terms, at = [], 0
				for ga in groups:
					terms.append(term(_lib.K_SE, [1.0 / float(v) for v in g[at:at + len(ga)]], cols=ga, k=kappa / len(groups)))
					at += len(ga)
			elif name == "matern":
				gamma = _scalar(arg['gamma']) if 'gamma' in arg else _scalar(owner.gamma)
				nu = arg['nu'] if 'nu' in arg else owner.v
				terms = [term(self._matern_kind(nu), [1.0 / gamma] * len(group), pname='gamma', pidx=[0] * len(group))]
			elif name == "ard_matern":
				g = vec(arg['ard_gamma'] if 'ard_gamma' in arg else owner.ard_gamma)
				nu = arg['nu'] if 'nu' in arg else owner.v
				terms = [term(self._matern_kind(nu), [1.0 / float(g[j]) for j in group], pname='ard_gamma', pidx=list(group))]  # kernels.py:941
			elif name in ("full_covariance_se", "full_covariance_matern"):
				# kernels.py:464-549: x[:, group] @ cov, then SE (gamma = 1) / Matern on Euclidean distances;
				# the Matern variant reads its smoothness from 'v' (not 'nu'), else the object's
				cov = arg['cov'] if 'cov' in arg else owner.cov
				cov = torch.as_tensor(cov).detach().double()
				kind = _lib.K_SE if name == "full_covariance_se" else self._matern_kind(arg['v'] if 'v' in arg else owner.v)
				terms = [term(kind, [1.0] * cov.shape[1], premap=cov, pname='cov')]
			elif name == "polynomial":
				degree = int(arg['degree'] if 'degree' in arg else owner.power)
				if degree != (arg['degree'] if 'degree' in arg else owner.power) or degree < 1:
					raise NotImplementedError("polynomial kernel: positive integer degrees only on the device")
				terms = [term(_lib.K_POLY | (degree << 8), [1.0] * len(group), offset=1.0)]  # kernels.py:760: (<b,a> + 1)^p
			elif name == "linear":
				offset = _scalar(arg['offset']) if 'offset' in arg else _scalar(owner.offset)
				terms = [term(_lib.K_LINEAR, [1.0] * len(group), offset=offset)]
			else:
				raise AssertionError("Kernel not implemented.")
			item = dict(op=self.operations[i], terms=terms)
			if len(terms) == 1:          # single-launch items keep the flat view the evidence-gradient code reads
				item.update(terms[0])
			items.append(item)
		return items

	@staticmethod
	def _matern_kind(nu):
		nu = _scalar(nu)
		if nu not in _MATERN_KIND:
			raise NotImplementedError("Matern nu=%s: only 0.5, 1.5, 2.5 run on the device (general-nu Bessel "
									  "form, kernels.py:852-858, is outside the hot path)" % nu)
		return _MATERN_KIND[nu]

	# ------------------------------------------------------------------ evaluation
	def _chain(self, kwargs=None, items=None):
		"""The resolved items of the expression (or the given sub-chain ``items``), the first one's operation taken as "set"."""
		if items is None:
			items = self._resolve(dict(kwargs) if kwargs else {})
		if items and items[0]['op'] != "-":
			items = [dict(items[0], op="-")] + list(items[1:])
		return items

	@staticmethod
	def _term_operands(term, x, dtype, device):
		"""(cols, inv_ls) of a launch of ``term`` on the points x, on the device: cols is None where the term reads every column of x
		in order -- also for x None: points that are the term's own coordinates already (pre-mapped), or that the launch does not read."""
		group = term['group']
		cols = None if x is None or group == list(range(x.shape[1])) else _dev_const(group, None, device, int32=True)
		return cols, _dev_const(term['inv_ls'], dtype, device)

	@staticmethod
	def _term_param_slots(term, device):
		"""pidx on the device: the entry of the term's hyper-parameter that sets each coordinate's lengthscale."""
		return _dev_const([int(v) for v in term['pidx']], None, device, int32=True)

	@staticmethod
	def _launches(items, out, diag_add=0.0):
		"""
		The one walk over a chain of items.  An item is the SUM of its terms, one launch each; items are chained with the + / *
		algebra of kernels.py:146-157.  Yields (term, target, combine, diag_add) for the caller to launch: target is ``out``, or for a
		multi-term item under "*" a scratch (allocated at the first such item) that the item is summed in and that is folded in,
		``out *= scratch``, after its last term.  ``diag_add`` rides on the last launch -- on the fold if the last launch folds.
		"""
		tmp, left = None, sum(len(it['terms']) for it in items)
		for it in items:
			comb = {"-": _lib.OUT_SET, "+": _lib.OUT_ADD, "*": _lib.OUT_MUL}[it['op']]
			fold = it['op'] == "*" and len(it['terms']) > 1
			if fold and tmp is None:
				tmp = torch.empty_like(out)
			for t_i, t in enumerate(it['terms']):
				left -= 1
				first = _lib.OUT_SET if fold else comb
				yield t, tmp if fold else out, first if t_i == 0 else _lib.OUT_ADD, diag_add if (left == 0 and not fold) else 0.0
			if fold and out.dim() == 1:          # (a diagonal folds as one row, and carries no noise term)
				_lib.combine(out.reshape(1, -1), tmp.reshape(1, -1), _lib.OUT_MUL)
			elif fold:
				_lib.combine(out, tmp, _lib.OUT_MUL, diag_add if left == 0 else 0.0)

	def _kernel_into(self, a, b, out, kwargs=None, diag_add=0.0, lower_only=False):
		"""
		Device-side evaluation: a (n, d), b (q, d) and out (q, n) are tensors on this process's
		GPU.  ``diag_add`` (s^2 of gauss_procc.py:151-163) is applied with the last launch.
		"""
		return self._run_items(self._chain(kwargs), a, b, out, diag_add, lower_only)

	def _run_items(self, items, a, b, out, diag_add=0.0, lower_only=False):
		"""Evaluates a chain of items into ``out`` with the operations as they stand: a first one other than "set" continues from
		the value ``out`` holds."""
		dmax = max(len(t['inv_ls']) for it in items for t in it['terms'])
		work = _lib.gram_workspace(a.shape[0], b.shape[0], dmax, out)          # one scratch for every launch
		same = a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride())
		for t, target, comb, dd in self._launches(items, out, diag_add):
			am, bm = a, b
			if t['premap'] is not None:
				am = self._premap(a, t['group'], t['premap'])
				bm = am if same else self._premap(b, t['group'], t['premap'])
			cols, inv_ls = self._term_operands(t, a if t['premap'] is None else None, out.dtype, out.device)
			_lib.gram(t['kind'], am, bm, target, inv_ls, cols, t['kappa'], t['offset'], diag_add=dd, lower_only=lower_only, combine=comb, work=work)
		return out

	def _combine_into(self, items, a, b, out, op, scratch=None):
		"""out (op)= the value of the chain ``items``, op one of _lib.OUT_SET / OUT_ADD / OUT_MUL.  A single item adds straight into
		``out`` and, if it is one term, multiplies straight into it (the combine of stpy_gram); anything else is evaluated into a
		scratch like ``out`` and combined by one stpy_combine.  Returns the scratch (``scratch`` if given, else allocated when needed)
		for the caller to pass to its next call."""
		if op == _lib.OUT_SET:
			self._run_items(self._chain(items=items), a, b, out)
		elif len(items) == 1 and (op == _lib.OUT_ADD or len(items[0]['terms']) == 1):
			self._run_items([dict(items[0], op="+" if op == _lib.OUT_ADD else "*")], a, b, out)
		else:
			if scratch is None:
				scratch = torch.empty_like(out)
			self._run_items(self._chain(items=items), a, b, scratch)
			_lib.combine(out, scratch, op)
		return scratch

	def _mul_factors_into(self, items, i, a, b, M, scratch=None):
		"""M *= everything item i is multiplied with (d K / d K_i, see ``_factors``); ``scratch`` as in ``_combine_into``."""
		for fac in self._factors(items, i):
			scratch = self._combine_into(fac, a, b, M, _lib.OUT_MUL, scratch)
		return scratch

	@staticmethod
	def _premap(x, group, cov):
		"""x[:, group] @ cov on the device (kernels.py:487-490) through the NT product: B = cov^T."""
		xg = x if group == list(range(x.shape[1])) else x[:, group]
		xg = xg.contiguous()
		ct = cov.to(device=x.device, dtype=x.dtype).t().contiguous()
		if ct.shape[1] != xg.shape[1]:
			raise ValueError("full-covariance kernel: cov has %d rows for %d selected columns" % (ct.shape[1], xg.shape[1]))
		out = torch.empty((xg.shape[0], ct.shape[0]), dtype=x.dtype, device=x.device)
		_lib.gemm_nt(xg, ct, out)
		return out

	def kernel(self, a, b, **kwargs):
		"""kernels.py:136-159.  a: (n, d), b: (q, d)  ->  (q, n); result lives where ``a`` lives."""
		ad = _lib.to_device(a)
		bd = _lib.to_device(b, ad.dtype)
		out = torch.empty((bd.shape[0], ad.shape[0]), dtype=ad.dtype, device=ad.device)
		self._kernel_into(ad, bd, out, kwargs)
		return _lib.like_input(out, a)

	def _diag_into(self, x, out, kwargs=None, items=None):
		for t, target, comb, _ in self._launches(self._chain(kwargs, items), out):
			# (a mapped stationary kernel has k(x, x) = kappa whatever the map; only dot-product kernels read x)
			cols, inv_ls = self._term_operands(t, x if t['premap'] is None else None, out.dtype, out.device)
			_lib.gram_diag(t['kind'], x, target, inv_ls, cols, t['kappa'], t['offset'], comb, d=None if t['premap'] is None else 0)
		return out

	def kernel_self_diag(self, x, **kwargs):
		"""k(x_i, x_i) for every row: what gauss_procc.py:347 assembles with a Python loop; shape (m,)."""
		xd = _lib.to_device(x)
		out = torch.empty((xd.shape[0],), dtype=xd.dtype, device=xd.device)
		self._diag_into(xd, out, kwargs)
		return _lib.like_input(out, x)

	# ------------------------------------------------------------------ input gradients (gauss_procc.py:420-459, :918-963)
	@staticmethod
	def _factors(items, i):
		"""The factors item i is multiplied with under the * algebra (d K / d K_i, as in the evidence gradient): the chain before it
		when its own operation is *, and every later item joined by *."""
		factors = []
		if items[i]['op'] == "*" and i > 0:
			factors.append(items[:i])
		for j in range(i + 1, len(items)):
			if items[j]['op'] == "*":
				factors.append([items[j]])
		return factors

	@staticmethod
	def _term_name(term):
		kind = term['kind'] & 0xff
		return {_lib.K_SE: "squared exponential", _lib.K_MATERN12: "Matern nu=0.5", _lib.K_MATERN32: "Matern nu=1.5",
				_lib.K_MATERN52: "Matern nu=2.5", _lib.K_LINEAR: "linear", _lib.K_POLY: "polynomial"}[kind] + \
			(" (full covariance)" if term['premap'] is not None else "")

	def _grad_into(self, x, xt, G, alpha=None, u=None, Wt=None, v=None, H=None, kwargs=None):
		"""
		G (m, D) <- d/dxt_t sum_i c_ti k(xt_t, x_i) with c_ti = u_t alpha_i + v_t Wt[t, i] (u / v None: 1; alpha or Wt None: that
		part is absent), and with H (m, D, D) also the second derivatives.  x (n, D), xt (m, D), Wt (m, >= n) are device tensors.
		Every term is one stpy_gram_grad launch that adds into G; the columns of a grouped term are scattered by the kernel.
		A full-covariance term is differentiated in the mapped coordinates z = x[:, group] cov and brought back by the chain rule
		(G[:, group] += G_z cov^T, one stpy_gemm_nt); the factors of a * item enter through the coefficients:
		C o prod_{l != j} K_l, formed with stpy_gram's multiply combine.
		"""
		items = self._chain(kwargs)
		if H is not None:
			for it in items:
				if it['op'] == "*":
					raise NotImplementedError("Hessian of a product kernel (item joined by '*') is not implemented on the device")
				for t in it['terms']:
					if t['kind'] in (_lib.K_MATERN12, _lib.K_MATERN32):
						raise NotImplementedError("Hessian of the %s term is not defined (singular at r = 0)" % self._term_name(t))
		G.zero_()
		if H is not None:
			H.zero_()
		m, n = xt.shape[0], x.shape[0]
		if m == 0 or n == 0:
			return G
		dev = G.device
		has_mul = any(it['op'] == "*" for it in items)
		C = None
		if has_mul:
			C = torch.zeros((m, n), dtype=G.dtype, device=dev)
			if alpha is not None:
				C += (u.reshape(-1, 1) if u is not None else 1.0) * alpha.reshape(1, -1)[:, :n]
			if Wt is not None:
				C += (v.reshape(-1, 1) if v is not None else 1.0) * Wt[:m, :n]
		tmp = None
		for i, it in enumerate(items):
			if not has_mul:
				coef = dict(alpha=alpha, u=u, Wt=Wt, v=v)
			elif self._factors(items, i):
				Ci = C.clone()
				tmp = self._mul_factors_into(items, i, x, xt, Ci, tmp)
				coef = dict(Wt=Ci)
			else:
				coef = dict(Wt=C)
			for t in it['terms']:
				self._term_grad(t, x, xt, coef, G, H)
		return G

	def _term_grad(self, t, x, xt, coef, G, H):
		"""One stpy_gram_grad launch of term t into G (H); coef: the alpha / u / Wt / v keywords of _lib.gram_grad."""
		m = xt.shape[0]
		dev = G.device
		if t['premap'] is not None:
			group = t['group']
			zx = self._premap(x, group, t['premap'])
			zt = self._premap(xt, group, t['premap'])
			p = zx.shape[1]
			Gz = torch.empty((m, p), dtype=G.dtype, device=dev)
			Hz = torch.empty((m, p, p), dtype=G.dtype, device=dev) if H is not None else None
			_lib.gram_grad(t['kind'], zx, zt, Gz, self._term_operands(t, None, G.dtype, dev)[1], None, t['kappa'], t['offset'], combine=_lib.OUT_SET, H=Hz, **coef)
			cov = t['premap'].to(device=dev, dtype=G.dtype).contiguous()            # (dg, p): G_z cov^T is the NT product of G_z and cov
			Gx = torch.empty((m, cov.shape[0]), dtype=G.dtype, device=dev)
			_lib.gemm_nt(Gz, cov, Gx)
			gi = torch.as_tensor(group, dtype=torch.long, device=dev)
			G.index_add_(1, gi, Gx)
			if H is not None:                   # cov H_z cov^T per point (d x d, single points): small, plumbing
				Hx = torch.einsum("ap,tpq,bq->tab", cov, Hz, cov)
				H[:, gi.reshape(-1, 1), gi.reshape(1, -1)] += Hx
			return
		cols, inv_ls = self._term_operands(t, x, G.dtype, dev)
		_lib.gram_grad(t['kind'], x, xt, G, inv_ls, cols, t['kappa'], t['offset'], combine=_lib.OUT_ADD, H=H, **coef)

	def _self_grad_into(self, xt, coef, G, kwargs=None):
		"""G[t] += coef_t * grad_x k(x, x) at x = xt_t: zero for stationary terms (k(x, x) = kappa); for the dot-product terms
		2 kappa phi'(s) inv_ls^2 x with s = |x * inv_ls|^2 (+ offset), the product rule over * items with the k(x, x) of the other
		factors (stpy_gram_diag).  O(m D) elementwise work on (m, D) tensors."""
		items = self._chain(kwargs)
		m = xt.shape[0]
		for i, it in enumerate(items):
			gi = None
			for t in it['terms']:
				kind = t['kind'] & 0xff
				if t['premap'] is not None or kind not in (_lib.K_LINEAR, _lib.K_POLY):
					continue
				cols = torch.as_tensor(t['group'], dtype=torch.long, device=xt.device)
				il = torch.as_tensor(t['inv_ls'], dtype=xt.dtype, device=xt.device)
				xs = xt[:, cols] * il
				if kind == _lib.K_LINEAR:
					f = torch.full((m, 1), 2.0 * t['kappa'], dtype=xt.dtype, device=xt.device)
				else:
					p = t['kind'] >> 8
					b = (xs * xs).sum(dim=1, keepdim=True) + t['offset']
					f = 2.0 * t['kappa'] * p * b ** (p - 1)
				g = torch.zeros_like(G)
				g[:, cols] = f * xs * il
				gi = g if gi is None else gi + g
			if gi is None:
				continue
			w = coef.reshape(-1, 1)
			for fac in self._factors(items, i):
				dv = torch.empty((m,), dtype=xt.dtype, device=xt.device)
				self._diag_into(xt, dv, items=fac)
				w = w * dv.reshape(-1, 1)
			G += w * gi
		return G

	# ------------------------------------------------------------------ finite-dimensional cases (kernels.py:263-273)
	def embed(self, x):
		if self.optkernel == "linear":
			return x
		raise AttributeError("This type of kernel does not support a finite dimensional embedding")

	def get_basis_size(self):
		if self.optkernel == "linear":
			return self.d
		raise AttributeError("This type of kernel does not support a finite dimensional embedding")
