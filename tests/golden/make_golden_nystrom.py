"""
Golden vectors of the Nystrom features: runs the REAL reference class (stpy/continuous_processes/nystrom_fea.py of a read-only
checkout of Mojusko/stpy) in the authoring container and stores inputs and its outputs as one small .npz fixture (arrays only).

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nystrom.py

As in make_golden.py, ``sys.modules`` is pre-seeded with inert placeholders for the optional solver packages the reference imports at
module top and this path never calls.  Two more notes:
* the module imports matplotlib at its top (visualize); a placeholder stands in when it is not installed;
* ``NystromFeatures.mean_std`` calls ``torch.solve(B, A)``, which current torch no longer has.  It returned (A^-1 B, LU); the shim below
  restores exactly that from torch.linalg.solve, so every stored number is still computed by the reference's own code.

N1_nystrom_uniform: approx="uniform", N = 200, d = 2, m = 8, gamma = 0.5, s = 0.1.  The data come from their own generator; the global
numpy seed is set immediately before fit_gp, so ``np.random.seed(seed); fit_gp(x, y)`` draws the stored C.  The seed is the first one
whose draw has no repeated index and whose landmark matrix has cond(K_mm) < 1e6.
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
try:
	import matplotlib.pyplot                                              # noqa: F401
except Exception:
	for name in ["matplotlib", "matplotlib.pyplot"]:
		sys.modules[name] = mock.MagicMock()
torch.solve = lambda B, A: (torch.linalg.solve(A, B), None)          # (current torch keeps the name only to raise)

from stpy.kernels import KernelFunction                                   # noqa: E402
from stpy.continuous_processes.nystrom_fea import NystromFeatures         # noqa: E402

N_PTS, DIM, M, GAMMA, S = 200, 2, 8, 0.5, 0.1


def main():
	path = os.path.join(HERE, "N1_nystrom_uniform.npz")
	if os.path.exists(path) and "--force" not in sys.argv:
		print("N1_nystrom_uniform.npz kept (exists; --force regenerates)")
		return
	rng = np.random.RandomState(20261019)
	x = rng.uniform(-1, 1, size=(N_PTS, DIM))
	y = np.sin(3 * x[:, :1]) * np.cos(2 * x[:, 1:2]) + S * rng.normal(size=(N_PTS, 1))
	xq = rng.uniform(-1, 1, size=(9, DIM))
	xt, yt, xqt = (torch.from_numpy(a).double() for a in (x, y, xq))
	for seed in range(1000):
		kernel = KernelFunction(kernel_name="squared_exponential", gamma=GAMMA, d=DIM)
		nys = NystromFeatures(kernel, m=M, approx="uniform", s=S)
		np.random.seed(seed)
		nys.fit_gp(xt, yt)
		C = np.asarray(nys.C)
		Kmm = kernel.kernel(xt[C, :], xt[C, :]).numpy()
		if len(set(C.tolist())) == M and np.linalg.cond(Kmm) < 1e6:
			break
	else:
		raise RuntimeError("no seed found")
	Eq, Ex = nys.embed(xqt), nys.embed(xt)
	mu, std = nys.mean_std(xqt)
	np.savez_compressed(path, x=x, y=y, C=C.astype(np.int64), xq=xq, seed=np.array(seed), gamma=np.array(GAMMA), s=np.array(S), m=np.array(M),
						gram_qq=(Eq @ Eq.T).numpy(), gram_qx=(Eq @ Ex.T).numpy(), mu=mu.numpy(), std=std.numpy())
	print("N1_nystrom_uniform.npz seed %d cond %.3g %.1f KB" % (seed, np.linalg.cond(Kmm), os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
	main()
