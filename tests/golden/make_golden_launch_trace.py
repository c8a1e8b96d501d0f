"""
Writes tests/golden/T1_launch_trace.json: the launch sequence (tests/launch_trace.py) of every (kernel expression, entry point) pair
of the catalogue below, recorded on the CPU.  tests/test_launch_trace_cpu.py records the same catalogue again and compares, so the
file pins WHAT is launched, in which order, on which operands -- not a value.

Regenerate only when a change to the launch plan is intended, from the repository root:

    python tests/golden/make_golden_launch_trace.py

and review the diff of the JSON (one line per entry) like code: every changed line is a changed launch sequence.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
	sys.path.insert(0, ROOT)

from stpy_amd.continuous_processes.gauss_procc import GaussianProcess          # noqa: E402
from stpy_amd.kernels import KernelFunction as KF                              # noqa: E402
from stpy_amd.parallel.block_cyclic import HipLocalOps                         # noqa: E402
from tests.launch_trace import launch_trace                                    # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "T1_launch_trace.json")
N, Q, D = 7, 5, 5
GROUPS = [[0, 1], [2, 3, 4]]


def _grid(rows, cols, p, q, r, m):
	i = torch.arange(rows, dtype=torch.float64).reshape(-1, 1)
	j = torch.arange(cols, dtype=torch.float64).reshape(1, -1)
	return (torch.remainder(p * i + q * j + r, m) / m).contiguous()


def data():
	"""Fixed operands (no random numbers: the small vectors are recorded by value)."""
	return dict(a=_grid(N, D, 3, 7, 1, 11), b=_grid(Q, D, 5, 2, 3, 13), y=_grid(N, 1, 4, 0, 2, 9), alpha=_grid(1, N, 0, 3, 1, 7).reshape(-1),
				u=_grid(1, Q, 0, 2, 1, 5).reshape(-1) + 0.5, v=_grid(1, Q, 0, 3, 2, 5).reshape(-1) - 0.25, Wt=_grid(Q, N + 1, 2, 3, 1, 17),
				coef=_grid(1, Q, 0, 4, 1, 7).reshape(-1))


# ---------------------------------------------------------------------------------------------- the expressions
def se(**kw):
	return KF(kernel_name="squared_exponential", gamma=0.8, kappa=1.5, d=D, **kw)


def ard(**kw):
	return KF(kernel_name="ard", ard_gamma=[0.5, 0.75, 1.0, 1.25, 1.5], kappa=0.5, d=D, **kw)


def ard_groups():
	return ard(groups=GROUPS)


def matern(nu=2.5):
	return KF(kernel_name="matern", gamma=1.25, nu=nu, d=D)


def linear():
	return KF(kernel_name="linear", offset=0.5, kappa=2.0, d=D)


def poly():
	return KF(kernel_name="polynomial", power=3, d=D)


def _cov(p):
	return _grid(D, p, 2, 3, 1, 7) + torch.eye(D, p, dtype=torch.float64)


def fc_se():
	return KF(kernel_name="full_covariance_se", cov=_cov(3), d=D)


def fc_matern():
	return KF(kernel_name="full_covariance_matern", cov=_cov(D), nu=2.5, d=D)


def _per_group(name, key, values):
	return lambda: {'0': {key: values, 'groups': GROUPS}}, lambda: KF(kernel_name=name, groups=GROUPS, d=D)


_SE_PG_KW, _SE_PG = _per_group("squared_exponential_per_group", "gamma_per_group", [0.5, 1.5])
_ARD_PG_KW, _ARD_PG = _per_group("ard_per_group", "ard_per_group", [0.5, 0.75, 1.0, 1.25, 1.5])

# name -> (constructor, constructor of the kwargs override every call gets, or None).  ``+`` / ``*`` modify their left operand, so
# every evaluation builds its expression anew.
EXPRESSIONS = {
	"se": (se, None),
	"se_group02": (lambda: se(group=[0, 2]), None),
	"ard": (ard, None),
	"matern52": (matern, None),
	"linear_offset": (linear, None),
	"poly3": (poly, None),
	"fc_se": (fc_se, None),
	"fc_matern": (fc_matern, None),
	"ard_groups": (ard_groups, None),
	"se_per_group": (_SE_PG, _SE_PG_KW),
	"ard_per_group": (_ARD_PG, _ARD_PG_KW),
	"se+ard": (lambda: se() + ard(), None),
	"ard_groups+poly3": (lambda: ard_groups() + poly(), None),
	"se*matern52": (lambda: se() * matern(), None),
	"se*ard_groups": (lambda: se() * ard_groups(), None),
	"ard_groups*se": (lambda: ard_groups() * se(), None),
	"(se+linear)*matern52": (lambda: (se() + linear()) * matern(), None),
	"se*matern52*ard": (lambda: se() * matern() * ard(), None),
	"se*fc_se+poly3": (lambda: se() * fc_se() + poly(), None),
	"ard_groups*matern52+fc_se*poly3": (lambda: ard_groups() * matern() + fc_se() * poly(), None),
	"se*matern52|gamma_override": (lambda: se() * matern(), lambda: {'0': {'gamma': 0.6}}),
}
HESSIAN_DEFINED = ("se", "se_group02", "ard", "matern52", "linear_offset", "poly3", "fc_se", "fc_matern", "ard_groups", "se_per_group",
				   "ard_per_group", "se+ard", "ard_groups+poly3")
# the evidence entry points evaluate the expression from its stored parameters: not the per-group kernels (their lengthscales exist
# only in an override) and not the entry that is about an override
EVIDENCE_DEFINED = tuple(k for k, (_, kw) in EXPRESSIONS.items() if kw is None)
BATCH_DEFINED = ("se", "se_group02", "matern52")


# ---------------------------------------------------------------------------------------------- the entry points
def _kernel_into_self(k, kw, t):
	out = torch.zeros((N, N), dtype=torch.float64)
	with launch_trace(a=t["a"], out=out) as tr:
		k._kernel_into(t["a"], t["a"], out, kw, diag_add=0.25, lower_only=True)
	return tr.launches


def _kernel_into_cross(k, kw, t):
	out = torch.zeros((Q, N), dtype=torch.float64)
	with launch_trace(a=t["a"], b=t["b"], out=out) as tr:
		k._kernel_into(t["a"], t["b"], out, kw)
	return tr.launches


def _diag_into(k, kw, t):
	out = torch.zeros((Q,), dtype=torch.float64)
	with launch_trace(x=t["b"], out=out) as tr:
		k._diag_into(t["b"], out, kw)
	return tr.launches


def _grad(k, kw, t, names, hessian=False):
	G = torch.ones((Q, D), dtype=torch.float64)
	H = torch.ones((Q, D, D), dtype=torch.float64) if hessian else None
	coef = {name: t[name] for name in names}
	with launch_trace(x=t["a"], xt=t["b"], G=G, H=H, **coef) as tr:
		k._grad_into(t["a"], t["b"], G, H=H, kwargs=kw, **coef)
	return tr.launches


def _self_grad_into(k, kw, t):
	G = torch.zeros((Q, D), dtype=torch.float64)
	with launch_trace(xt=t["b"], coef=t["coef"], G=G) as tr:
		k._self_grad_into(t["b"], t["coef"], G, kwargs=kw)
	return tr.launches


def _local_gram(add):
	def run(k, kw, t):
		wide = torch.ones((Q, N + 4), dtype=torch.float64)
		out = wide[:, 2:2 + N]
		with launch_trace(xa=t["a"], xb=t["b"], out=out) as tr:
			HipLocalOps().gram(k, t["a"], t["b"], out, kw, add=add)
		return tr.launches
	return run


def _evidence_gradient(k, kw, t):
	"""fit_gp, then log_marginal(kernel, X, 1.0).backward() with every gamma / ard_gamma / cov of X and the noise requiring grad."""
	X = {}
	for key, params in k.params_dict.items():
		X[key] = dict(params)
		for name in ("gamma", "ard_gamma", "cov"):
			if name in params:
				X[key][name] = torch.as_tensor(params[name]).detach().double().clone().requires_grad_(True)
	with launch_trace(x=t["a"], y=t["y"]) as tr:
		gp = GaussianProcess(kernel=k, s=torch.tensor([0.1], dtype=torch.float64, requires_grad=True))
		gp.fit_gp(t["a"], t["y"])
		gp.log_marginal(k, X, 1.0).backward()
	return tr.launches


def _evidence_after_load_data(k, kw, t):
	with launch_trace(x=t["a"], y=t["y"]) as tr:
		gp = GaussianProcess(kernel=k, s=0.1)
		gp.load_data((t["a"], t["y"]))
		gp.log_marginal(k, {}, torch.tensor(0.5))
	return tr.launches


def _evidence_batch(k, kw, t):
	Xs = [{'0': {'gamma': torch.tensor([g], dtype=torch.float64)}} for g in (0.5, 0.9)]
	with launch_trace(x=t["a"], y=t["y"]) as tr:
		gp = GaussianProcess(kernel=k, s=0.1)
		gp.load_data((t["a"], t["y"]))
		gp.log_marginal_batch(k, Xs, 1.0, s=[0.1, 0.2])
		assert gp.lml_batch_path == "device"
	return tr.launches


ALL = tuple(EXPRESSIONS)
ENTRY_POINTS = {
	"kernel_into_self": (_kernel_into_self, ALL),
	"kernel_into_cross": (_kernel_into_cross, ALL),
	"diag_into": (_diag_into, ALL),
	"grad_into_alpha": (lambda k, kw, t: _grad(k, kw, t, ("alpha",)), ALL),
	"grad_into_alpha_u_Wt_v": (lambda k, kw, t: _grad(k, kw, t, ("alpha", "u", "Wt", "v")), ALL),
	"grad_into_hessian": (lambda k, kw, t: _grad(k, kw, t, ("alpha",), hessian=True), HESSIAN_DEFINED),
	"self_grad_into": (_self_grad_into, ALL),
	"local_gram": (_local_gram(False), ALL),
	"local_gram_add": (_local_gram(True), ALL),
	"evidence_gradient": (_evidence_gradient, EVIDENCE_DEFINED),
	"evidence_after_load_data": (_evidence_after_load_data, ("se", "se*ard_groups")),
	"evidence_batch": (_evidence_batch, BATCH_DEFINED),
}


def entries():
	"""[(id, function without arguments that records and returns the launches)], in a fixed order."""
	out = []
	for expr, (make, make_kw) in EXPRESSIONS.items():
		for entry, (run, defined) in ENTRY_POINTS.items():
			if expr in defined:
				out.append(("%s/%s" % (expr, entry), lambda run=run, make=make, make_kw=make_kw: run(make(), make_kw() if make_kw else None, data())))
	return out


def record(fn):
	"""The launches as JSON holds them (tuples become lists; a NaN would be a recorded value that no launch defines)."""
	return json.loads(json.dumps(fn(), allow_nan=False))


def main():
	lines = ['"%s": %s' % (name, json.dumps(fn(), allow_nan=False, separators=(",", ":"))) for name, fn in entries()]
	with open(PATH, "w") as fh:
		fh.write("{\n" + ",\n".join(lines) + "\n}\n")
	print("wrote %s: %d entries, %d bytes" % (PATH, len(lines), os.path.getsize(PATH)))


if __name__ == "__main__":
	main()
