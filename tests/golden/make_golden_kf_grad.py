"""
Golden vectors of the feature-space posterior's input gradients (G18): runs the REAL reference (Mojusko/stpy, a read-only checkout
on PYTHONPATH) on the CPU in the authoring container, in the style of make_golden_grad.py, and stores inputs + the reference's
outputs.

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kf_grad.py

Every gradient below is the reference's autograd through KernelizedFeatures.mean_std (kernelized_features.py:269-288, :441-456) in
fp64; the Jacobians are QuadratureEmbedding.derivative_1 / derivative_2 (embedding.py:268-304).  The same placeholder modules as
make_golden.py stand in for the optional solver packages the squared-loss path never calls.

CASES describes every model; tests/test_kf_input_grad.py repeats the table to build the same models.
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

S_NOISE, LAM = 0.2, 1.3
# case -> (embedding class, its keyword arguments, training points, primal)
CASES = {
	"rff": ("RFFEmbedding", dict(gamma=0.8, m=32, d=3, kappa=1.5), 120, True),
	"hermite": ("HermiteEmbedding", dict(gamma=0.5, m=2 * 6 ** 2, d=2, kappa=1.2), 120, True),
	"dual": ("RFFEmbedding", dict(gamma=0.8, m=32, d=3, kappa=1.5), 20, False),
}


def main():
	import stpy.embeddings.embedding as E                                                    # noqa: E402
	from stpy.continuous_processes.kernelized_features import KernelizedFeatures             # noqa: E402

	def T(a):
		return torch.from_numpy(np.ascontiguousarray(a)).double()

	def N(t):
		return t.detach().numpy().copy()

	rng = np.random.RandomState(20250307)
	W_rff = rng.normal(size=(32, 3)) / 0.8
	out = {"rff_W": W_rff}
	for case, (cls, kw, ntrain, primal) in CASES.items():
		d = kw["d"]
		x = rng.uniform(-1, 1, size=(ntrain, d))
		y = np.sin(2 * x[:, :1]) + x[:, 1:2] * x[:, -1:] + 0.1 * rng.normal(size=(ntrain, 1))
		xb = rng.uniform(-1, 1, size=(6, d))
		pts = rng.uniform(-1, 1, size=(4, d))
		emb = getattr(E, cls)(**kw)
		if cls == "RFFEmbedding":
			emb.W = T(W_rff)
		KF = KernelizedFeatures(embedding=emb, m=emb.get_m(), s=S_NOISE, lam=LAM, d=d, primal=primal)
		KF.fit_gp(T(x), T(y))
		assert bool(KF.dual) == (not primal)
		out[case + "_x"], out[case + "_y"], out[case + "_xb"], out[case + "_pts"] = x, y, xb, pts
		xt = T(xb).requires_grad_(True)
		mu, std = KF.mean_std(xt)
		mu.sum().backward()
		out[case + "_mu"], out[case + "_dmu_sum"] = N(mu), N(xt.grad)
		xt = T(xb).requires_grad_(True)
		mu, std = KF.mean_std(xt)
		std.sum().backward()
		out[case + "_std"], out[case + "_dstd_sum"] = N(std), N(xt.grad)
		grads, hess = [], []
		for p in pts:
			g, h = KF.mean_gradient_hessian(T(p.reshape(1, d)), hessian=True)
			grads.append(N(g))
			hess.append(N(h))
		out[case + "_grad"], out[case + "_hess"] = np.stack(grads), np.stack(hess)
		theta, Z = KF.theta_mean(var=True)
		out[case + "_theta"], out[case + "_Z"] = N(theta), N(Z)
		if cls == "HermiteEmbedding":
			out[case + "_d1"] = N(emb.derivative_1(T(xb)))
			out[case + "_d2"] = N(emb.derivative_2(T(xb)))
	path = os.path.join(HERE, "G18_kf_input_grad.npz")
	if os.path.exists(path) and "--force" not in sys.argv:
		print("G18_kf_input_grad.npz kept (exists; --force regenerates)")
		return
	np.savez_compressed(path, s=np.array(S_NOISE), lam=np.array(LAM), **out)
	print("G18_kf_input_grad.npz %7.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
	main()
