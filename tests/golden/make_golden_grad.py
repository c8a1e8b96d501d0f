"""
Golden vectors of the posterior's input gradients (G17): runs the REAL reference (Mojusko/stpy, read-only at
/root/reference) in the authoring container, in the style of make_golden.py, and stores inputs + the reference's outputs.

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grad.py

The reference differentiates its posterior by autograd through mean_std (gauss_procc.py:420-459 mean_gradient_hessian,
tests/gradients_test.py): every number below is that autograd result on the CPU, in fp64.  The same placeholder modules as
make_golden.py stand in for the optional solver packages the squared-loss path never calls.

CASES describes every kernel; tests/test_posterior_grad.py repeats the table to build the same kernels.
"""
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

for name in ["cvxpy", "cvxpylayers", "cvxpylayers.torch", "pymanopt", "pymanopt.manifolds",
			 "pymanopt.optimizers", "pymanopt.function", "torchmin", "autograd_minimize", "mosek"]:
	if name not in sys.modules:
		sys.modules[name] = mock.MagicMock()

D = 3
COV = [[0.9, 0.2, 0.0], [-0.1, 1.3, 0.3], [0.2, 0.0, 0.7]]
# case -> list of (operation, constructor keyword arguments) of KernelFunction; the first operation is "-"
CASES = {
	"se": [("-", dict(kernel_name="squared_exponential", gamma=0.7, kappa=1.3))],
	"ard": [("-", dict(kernel_name="ard", ard_gamma=[0.5, 0.9, 1.4], kappa=1.1))],
	"ard_groups": [("-", dict(kernel_name="ard", ard_gamma=[0.6, 0.8, 1.2], kappa=1.1, groups=[[0, 1], [2]]))],
	"se_plus_linear": [("-", dict(kernel_name="squared_exponential", gamma=0.8, kappa=1.0)),
					   ("+", dict(kernel_name="linear", kappa=0.5))],
	"se_times_se": [("-", dict(kernel_name="squared_exponential", gamma=0.8, kappa=1.0)),
					("*", dict(kernel_name="squared_exponential", gamma=2.0, kappa=0.7, group=[1, 2]))],
	"poly": [("-", dict(kernel_name="polynomial", power=3, kappa=0.4))],
	"fullcov_se": [("-", dict(kernel_name="full_covariance_se", cov=COV, kappa=1.2))],
}
S_NOISE = 0.1


def make_kernel(KernelFunction, spec, tensor):
	k = None
	for op, kw in spec:
		kw = dict(kw, d=D)
		if "ard_gamma" in kw:
			kw["ard_gamma"] = tensor(kw["ard_gamma"])
		if "cov" in kw:
			kw["cov"] = tensor(kw["cov"])
		item = KernelFunction(**kw)
		k = item if k is None else (k + item if op == "+" else k * item)
	return k


def main():
	from stpy.kernels import KernelFunction                                   # noqa: E402
	from stpy.continuous_processes.gauss_procc import GaussianProcess         # noqa: E402

	def T(a):
		return torch.from_numpy(np.ascontiguousarray(a)).double()

	def N(t):
		return t.detach().numpy().copy()

	rng = np.random.RandomState(20241117)
	x = rng.uniform(-1, 1, size=(40, D))
	y = np.sin(2 * x[:, :1]) + x[:, 1:2] * x[:, 2:3] + 0.1 * rng.normal(size=(40, 1))
	pts = rng.uniform(-1, 1, size=(4, D))
	xb = rng.uniform(-1, 1, size=(6, D))
	out = {}
	for case, spec in CASES.items():
		GP = GaussianProcess(kernel=make_kernel(KernelFunction, spec, lambda v: torch.tensor(v, dtype=torch.float64)), s=S_NOISE, d=D)
		GP.fit_gp(T(x), T(y))
		grads, hess = [], []
		for p in pts:
			g, h = GP.mean_gradient_hessian(T(p.reshape(1, D)), hessian=True)
			grads.append(N(g))
			hess.append(N(h))
		out[case + "_grad"] = np.stack(grads)
		out[case + "_hess"] = np.stack(hess)
		xt = T(xb).requires_grad_(True)
		mu, std = GP.mean_std(xt)
		mu.sum().backward()
		out[case + "_mu"] = N(mu)
		out[case + "_dmu_sum"] = N(xt.grad)
		xt = T(xb).requires_grad_(True)
		mu, std = GP.mean_std(xt)
		std.sum().backward()
		out[case + "_std"] = N(std)
		out[case + "_dstd_sum"] = N(xt.grad)
	path = os.path.join(HERE, "G17_posterior_grad.npz")
	if os.path.exists(path) and "--force" not in sys.argv:
		print("G17_posterior_grad.npz kept (exists; --force regenerates)")
		return
	np.savez_compressed(path, x=x, y=y, pts=pts, xb=xb, s=np.array(S_NOISE), **out)
	print("G17_posterior_grad.npz %7.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
	main()
