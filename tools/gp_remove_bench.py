"""Row deletion from the resident factor on the MI355X, one process, device events:
 (a) stpy_potrf_delete (through its typed wrapper; destination and winv allocated once) for k = 1 / 32 / 128 consecutive rows at the
     oldest, the middle and the newest end of the data, against GaussianProcess.fit_gp of the same N (the refit a deletion replaces);
 (b) one step of a sliding window -- add_data_point + remove_data_point(0) + mean_std on 4096 points -- with iterative=True
     (stpy_potrf_append, stpy_potrf_delete) against the same step with iterative=False (two refits: the only route before
     remove_data_point existed), each part timed on its own.
Data: U(0,1)^3, SE gamma = 0.5, s = 0.3 (the recipe of tests/test_gp_append.py), N = 4096 / 16 384 / 32 768, fp64 and fp32.
usage: python tools/gp_remove_bench.py [quick]      (quick: N = 4096 only)"""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from stpy_amd import GaussianProcess, _lib as L          # noqa: E402


def event_ms(f, reps=3, setup=None):
	"""min and median device time (ms) of f() over ``reps`` runs after one warm-up; ``setup`` runs before each, outside the window."""
	ts = []
	for rep in range(reps + 1):
		if setup is not None:
			setup()
		torch.cuda.synchronize()
		e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		e0.record()
		f()
		e1.record()
		e1.synchronize()
		if rep > 0:
			ts.append(e0.elapsed_time(e1))
	return min(ts), float(np.median(ts))


def data(n, dtype, dev, seed=11):
	g = torch.Generator().manual_seed(seed)
	x = torch.rand((n, 3), generator=g, dtype=torch.float64)
	y = torch.sin(4 * x[:, :1]) + 0.1 * torch.randn((n, 1), generator=g, dtype=torch.float64)
	return x.to(device=dev, dtype=dtype), y.to(device=dev, dtype=dtype)


def gp():
	return GaussianProcess(gamma=0.5, s=0.3, kappa=1.0, kernel_name="squared_exponential", d=3)


def call_part(n, dtype, dev):
	x, y = data(n, dtype, dev)
	GP = gp()
	fit = event_ms(lambda: GP.fit_gp(x, y))
	A = GP._L
	B = torch.empty_like(A)
	winv = torch.empty((L.potrf_winv_elems(A.shape[0]),), dtype=dtype, device=dev)
	name = "fp64" if dtype == torch.float64 else "fp32"
	print("| %s | %d | fit_gp (refit) | - | %.2f | %.2f | 1.0 |" % (name, n, fit[0], fit[1]), flush=True)
	for k in (1, 32, 128):
		for where, first in (("oldest", 0), ("middle", n // 2), ("newest", n - k)):
			S = list(range(first, first + k))
			t = event_ms(lambda: L.potrf_delete(A, n, S, B, winv))
			print("| %s | %d | delete %s | %d | %.2f | %.2f | %.1f |" % (name, n, where, k, t[0], t[1], fit[0] / t[0]), flush=True)
	del GP, A, B, winv


def window_part(n, dtype, dev, m=4096):
	x, y = data(n + 16, dtype, dev)
	xt = data(m, dtype, dev, seed=9)[0]
	name = "fp64" if dtype == torch.float64 else "fp32"
	for iterative in (True, False):
		GP = gp()
		GP.fit_gp(x[:n], y[:n])
		state = {"t": 0}

		def add():
			t = state["t"]
			GP.add_data_point(x[n + t:n + t + 1], y[n + t:n + t + 1], iterative=iterative)
			state["t"] = (t + 1) % 16

		def remove():
			GP.remove_data_point(0, iterative=iterative)

		def predict():
			GP.mean_std(xt)

		def step():
			add()
			remove()
			predict()
		step()                                        # (the first append grows the capacity buffer once)
		ta = event_ms(add, setup=None)
		# (the window now holds n + 4 points; bring it back to n so that remove / predict are timed at the size of the step)
		for _ in range(4):
			remove()
		tr = event_ms(remove, setup=add)
		tp = event_ms(predict)
		ts = event_ms(step)
		print("| %s | %d | %s | %.2f | %.2f | %.2f | %.2f | %s |" % (name, n, "iterative=True" if iterative else "iterative=False (refits)",
																	 ta[0], tr[0], tp[0], ts[0], GP.remove_path), flush=True)
		del GP


def main():
	dev = torch.device("cuda:0")
	sizes = (4096,) if "quick" in sys.argv[1:] else (4096, 16384, 32768)
	print("# library %s" % L.load().stpy_version().decode())
	print("# (a) stpy_potrf_delete against the refit; ms, min (median) of 3 after a warm-up")
	print("| dtype | N | call | k | min ms | median ms | refit / call |")
	print("|---|---|---|---|---|---|---|")
	for dtype in (torch.float64, torch.float32):
		for n in sizes:
			call_part(n, dtype, dev)
	print("# (b) one sliding-window step at N points, 4096 test points; ms, min of 3 after a warm-up")
	print("| dtype | N | route | add_data_point | remove_data_point(0) | mean_std | whole step | remove_path |")
	print("|---|---|---|---|---|---|---|---|")
	for dtype in (torch.float64, torch.float32):
		for n in sizes:
			window_part(n, dtype, dev)


if __name__ == "__main__":
	main()
