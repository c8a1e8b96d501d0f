"""Input gradients of the feature-space posterior on the MI355X, one process, device events:
 (a) stpy_rff_grad order 1 (per-point coefficients, values requested; and the shared row) against stpy_rff_embed of the same
     (n, d, m, dtype) in the same run, alternating;
 (b) KernelizedFeatures.mean_std + backward of mu.sum() + std.sum() against mean_std alone (primal, m = 8192 features, 4096 test points);
 (c) sample_and_optimize, m = 8192, d = 4, 25 starts: wall time and device evaluations.
usage: python tools/kf_grad_bench.py [quick]      (quick: the n = 4096 shapes of (a) only)"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from stpy_amd import RFFEmbedding, _lib as L                                               # noqa: E402
from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures           # noqa: E402


def event_ms(fns, reps=7):
	"""min and median device time (ms) of each callable, the callables alternating inside every repetition."""
	for f in fns:
		f()
	torch.cuda.synchronize()
	ts = [[] for _ in fns]
	for _ in range(reps):
		for k, f in enumerate(fns):
			e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			e0.record()
			f()
			e1.record()
			e1.synchronize()
			ts[k].append(e0.elapsed_time(e1))
	return [(min(t), float(np.median(t))) for t in ts]


def kernel_part(dev, quick):
	lib = L.load()
	print("# (a) stpy_rff_grad against stpy_rff_embed, library %s" % lib.stpy_version().decode(), flush=True)
	print("# dtype n m d | grad per-point C ms (median) C read GB/s | grad shared row ms | embed ms (median) write GB/s | ratio grad/embed")
	for dtype in (torch.float64, torch.float32):
		esz = 8 if dtype == torch.float64 else 4
		for n in ((4096,) if quick else (4096, 25600)):
			for m in (8192, 32768):
				for d in (16, 64):
					g = torch.Generator().manual_seed(n + m + d)
					x = (torch.rand((n, d), generator=g, dtype=torch.float64) * 2 - 1).to(device=dev, dtype=dtype)
					W = (torch.randn((m, d), generator=g, dtype=torch.float64) / (0.5 * d ** 0.5)).to(device=dev, dtype=dtype)
					C = torch.randn((n, m), dtype=dtype, device=dev)
					row = C[0].contiguous()
					G = torch.empty((n, d), dtype=dtype, device=dev)
					val = torch.empty((n,), dtype=dtype, device=dev)
					dt = L.dtype_code(dtype)
					work = torch.empty((max(int(lib.stpy_rff_grad_workspace_bytes(dt, n, d, m, 1)), 1),), dtype=torch.uint8, device=dev)
					out = torch.empty((n, m), dtype=dtype, device=dev)
					wb = int(lib.stpy_rff_workspace_bytes(dt, n, d, m))
					ework = torch.empty((max(wb, 1),), dtype=torch.uint8, device=dev)
					scale = (2.0 / m) ** 0.5

					def grad(Cm=C, ldc=m):
						L.check(lib.stpy_rff_grad(dt, L.ptr(x), n, d, d, L.ptr(W), d, m, None, None, scale, L.ptr(Cm), ldc, 1, L.OUT_SET, L.ptr(val), L.ptr(G), d,
												  None, L.ptr(work), work.numel(), L.stream_ptr()), "stpy_rff_grad")

					def embed():
						L.check(lib.stpy_rff_embed(dt, L.ptr(x), n, d, d, L.ptr(W), d, m, None, None, scale, L.ptr(out), m, 0, L.ptr(ework) if wb else None, wb,
												   L.stream_ptr()), "stpy_rff_embed")
					(tg, tgm), (ts, _), (te, tem) = event_ms([grad, lambda: grad(row, 0), embed])
					print("%s n=%d m=%d d=%d | %.3f (%.3f) %.0f | %.3f | %.3f (%.3f) %.0f | %.2f" % (
						"fp64" if esz == 8 else "fp32", n, m, d, tg, tgm, n * m * esz / tg / 1e6, ts, te, tem, n * m * esz / te / 1e6, tg / te), flush=True)
					del C, out, work, ework


def estimator_part(dev):
	print("# (b) mean_std + backward against mean_std: primal, m = 8192 features, d = 16, 8192 training points, 4096 test points, fp64", flush=True)
	rng = np.random.RandomState(0)
	d, m = 16, 8192
	np.random.seed(1)
	emb = RFFEmbedding(gamma=d ** 0.5, m=m, d=d)
	x = torch.from_numpy(rng.uniform(-1, 1, size=(8192, d))).to(dev)
	y = torch.sin(x.sum(1, keepdim=True))
	KF = KernelizedFeatures(embedding=emb, m=m, s=0.1, lam=1.0, d=d)
	KF.fit_gp(x, y)
	xt = torch.from_numpy(rng.uniform(-1, 1, size=(4096, d))).to(dev)

	def forward():
		KF.mean_std(xt)

	def both():
		z = xt.clone().requires_grad_(True)
		mu, std = KF.mean_std(z)
		(mu.sum() + std.sum()).backward()

	def mean_only():
		z = xt.clone().requires_grad_(True)
		KF.mean(z).sum().backward()
	both()                                        # V^-1 once per fit (stpy_potri), outside the timed window
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	KF._factor._inverse = None
	KF._factor.inverse()
	torch.cuda.synchronize()
	print("V^-1 (stpy_potri, once per fit) m=%d: %.1f ms" % (m, (time.perf_counter() - t0) * 1e3))
	(tf, tfm), (tb, tbm), (tm, tmm) = event_ms([forward, both, mean_only], reps=5)
	print("mean_std                       : %.2f ms (median %.2f)" % (tf, tfm))
	print("mean_std + backward(mu + std)  : %.2f ms (median %.2f)  ratio %.2f" % (tb, tbm, tb / tf))
	print("mean + backward(mu)            : %.2f ms (median %.2f)  ratio %.2f" % (tm, tmm, tm / tf), flush=True)


def optimize_part(dev):
	print("# (c) sample_and_optimize: m = 8192 features, d = 4, 4096 training points, 25 starts, fp64", flush=True)
	rng = np.random.RandomState(0)
	xs = rng.uniform(-1, 1, size=(4096, 4))
	ys = np.sin(3 * xs[:, :1]) * np.cos(2 * xs[:, 1:2]) + 0.1 * rng.normal(size=(4096, 1))
	np.random.seed(2)
	emb = RFFEmbedding(gamma=0.5, m=8192, d=4)
	KF = KernelizedFeatures(embedding=emb, m=8192, s=0.1, lam=1.0, d=4, bounds=[(-1.0, 1.0)] * 4)
	KF.fit_gp(torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev))
	for trial in range(2):                        # the first call also pays the sampler's one-off work (V^-1, its factor)
		torch.manual_seed(trial)
		np.random.seed(trial)
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		sol, val = KF.sample_and_optimize(multistart=25)
		t = time.perf_counter() - t0
		print("sample_and_optimize call %d: %.3f s, %d device evaluations, value %.6f at %s" % (
			trial, t, KF._last_optimize_evaluations, float(val[0]), np.array2string(sol.numpy(), precision=4)), flush=True)


def main():
	dev = torch.device("cuda:0")
	kernel_part(dev, "quick" in sys.argv[1:])
	estimator_part(dev)
	optimize_part(dev)


if __name__ == "__main__":
	main()
