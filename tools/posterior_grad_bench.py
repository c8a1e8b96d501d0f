"""Input gradients of the GP posterior on the MI355X: stpy_gram_grad against stpy_gram on the same M x N (fp64, d = 16), mean_std_grad
against mean_std at the headline shape, and ucb_optimize wall time.
usage: python tools/posterior_grad_bench.py [N] [M]      (defaults 65536 4096; the ucb_optimize problem is N = 4096, d = 4, 25 starts)"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from stpy_amd import GaussianProcess, _lib as L                  # noqa: E402


def timed(fn, reps=5):
	fn()
	torch.cuda.synchronize()
	ts = []
	for _ in range(reps):
		t0 = time.perf_counter()
		fn()
		torch.cuda.synchronize()
		ts.append(time.perf_counter() - t0)
	return min(ts), float(np.median(ts))


def main():
	n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
	m = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
	d = 16
	dev = torch.device("cuda:0")
	lib = L.load()
	g = torch.Generator().manual_seed(1)
	x = (torch.rand(n, d, generator=g, dtype=torch.float64) * 2 - 1).to(dev)
	xt = (torch.rand(m, d, generator=g, dtype=torch.float64) * 2 - 1).to(dev)
	il = torch.full((d,), 1.0 / d ** 0.5, dtype=torch.float64, device=dev)
	alpha = torch.randn(n, dtype=torch.float64, device=dev)
	u = torch.randn(m, dtype=torch.float64, device=dev)
	v = torch.randn(m, dtype=torch.float64, device=dev)
	Wt = torch.randn((m, n), dtype=torch.float64, device=dev)
	G = torch.empty((m, d), dtype=torch.float64, device=dev)
	work = torch.empty((int(lib.stpy_gram_grad_workspace_bytes(L.F64, m, n, d, 1)),), dtype=torch.uint8, device=dev)

	def grad():
		L.check(lib.stpy_gram_grad(L.K_SE, L.F64, L.ptr(x), n, d, L.ptr(xt), m, d, d, None, L.ptr(il), 1.0, 0.0, L.ptr(alpha), L.ptr(u), L.ptr(Wt), n,
								   L.ptr(v), 1, L.OUT_SET, L.ptr(G), d, None, L.ptr(work), work.numel(), L.stream_ptr()), "stpy_gram_grad")
	K = torch.empty((m, n), dtype=torch.float64, device=dev)
	gw = torch.empty((int(lib.stpy_gram_workspace_bytes(L.F64, n, m, d)),), dtype=torch.uint8, device=dev)

	def gram():
		L.check(lib.stpy_gram(L.K_SE, L.F64, L.ptr(x), n, d, L.ptr(xt), m, d, d, None, L.ptr(il), 1.0, 0.0, 0.0, 0, L.OUT_SET, L.ptr(K), n,
							  L.ptr(gw), gw.numel(), L.stream_ptr()), "stpy_gram")
	tg, tgm = timed(grad)
	tk, tkm = timed(gram)
	print("stpy_gram_grad order 1 + Wt  M=%d N=%d d=16 fp64: %.3f ms (median %.3f)  Wt read %.0f GB/s" % (m, n, tg * 1e3, tgm * 1e3, m * n * 8 / tg / 1e9), flush=True)
	print("stpy_gram (MFMA fill)        M=%d N=%d d=16 fp64: %.3f ms (median %.3f)  write %.0f GB/s  ratio grad/gram %.2f" % (m, n, tk * 1e3, tkm * 1e3, m * n * 8 / tk / 1e9, tg / tk), flush=True)
	del Wt, K, gw, work

	y = torch.sin(x.sum(1, keepdim=True))
	gp = GaussianProcess(gamma=d ** 0.5, s=0.1, kernel_name="squared_exponential", d=d)
	gp.fit_gp(x, y)
	torch.cuda.synchronize()
	gp.mean_std_grad(xt[:8])                     # builds the reversed factor once (per fit)
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	gp._factor._reversed = None
	gp._factor.reversed()
	torch.cuda.synchronize()
	print("reversed factor (stpy_trsm_ln_factor) N=%d: %.2f ms" % (n, (time.perf_counter() - t0) * 1e3), flush=True)
	ts, tsm = timed(lambda: gp.mean_std(xt), reps=3)
	td, tdm = timed(lambda: gp.mean_std_grad(xt), reps=3)
	print("mean_std      N=%d M=%d: %.1f ms (median %.1f)" % (n, m, ts * 1e3, tsm * 1e3))
	print("mean_std_grad N=%d M=%d: %.1f ms (median %.1f)  ratio %.2f" % (n, m, td * 1e3, tdm * 1e3, td / ts), flush=True)
	del gp

	rng = np.random.RandomState(0)
	xs = rng.uniform(-1, 1, size=(4096, 4))
	ys = np.sin(3 * xs[:, :1]) * np.cos(2 * xs[:, 1:2]) + 0.1 * rng.normal(size=(4096, 1))
	gp = GaussianProcess(gamma=0.5, s=0.1, kernel_name="squared_exponential", d=4, bounds=[(-1.0, 1.0)] * 4)
	gp.fit_gp(torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev))
	np.random.seed(0)
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	sol, val = gp.ucb_optimize(2.0, multistart=25)
	t = time.perf_counter() - t0
	print("ucb_optimize N=4096 d=4 multistart=25: %.3f s  value %.6f at %s" % (t, float(val), np.array2string(sol.numpy(), precision=4)))


if __name__ == "__main__":
	main()
