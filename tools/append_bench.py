"""Bordered Cholesky append (stpy_potrf_append) on the MI355X.
  1. N0 = 65 536, fp64, d = 16: one append of k rows (k = 1, 4, 16, 64, 256; the whole C ABI call, the Gram rows excluded) against
     the full refit (GaussianProcess.fit_gp on N0 + k points) and against one stpy_trsv of order N0;
  2. the crossover: the same append on the dataflow solve and on the MFMA block solve (stpy_tune key 34) for k = 8 .. 128;
  3. N0 = 16 384: 128 iterations of (add one point + mean_std on 4096 candidates), add_data_point(iterative=True) against the refit.
usage: python tools/append_bench.py [N0]      (default 65536; section 3 always runs at 16 384)"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from stpy_amd import GaussianProcess, _lib as L                  # noqa: E402

IB = 128


def pad(n):
	return -(-int(n) // IB) * IB


def ev_time(fn, reps=5, before=None):
	"""median device time (ms) of fn over reps runs; before() runs untimed in front of each"""
	ts = []
	for _ in range(reps + 1):
		if before:
			before()
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		a.record()
		fn()
		b.record()
		torch.cuda.synchronize()
		ts.append(a.elapsed_time(b))
	return float(np.median(ts[1:]))


def main():
	n0 = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
	d, kmax = 16, 256
	dev = torch.device("cuda:0")
	lib = L.load()
	g = torch.Generator().manual_seed(1)
	x = torch.rand(n0 + kmax, d, generator=g, dtype=torch.float64).to(dev)
	y = torch.randn(n0 + kmax, 1, generator=g, dtype=torch.float64).to(dev)
	GP = GaussianProcess(gamma=1.0, s=0.3, kernel_name="squared_exponential", d=d)
	t = time.perf_counter()
	GP.fit_gp(x[:n0], y[:n0])
	torch.cuda.synchronize()
	fit_ms = (time.perf_counter() - t) * 1e3
	# the factor in a buffer with room for kmax more rows (what add_data_point(iterative=True) holds after a growth)
	cap = pad(n0 + kmax)
	A = torch.zeros((cap, cap), dtype=torch.float64, device=dev)
	A[:GP._L.shape[0], :GP._L.shape[0]] = GP._L
	winv = torch.empty((int(lib.stpy_potrf_winv_elems(cap)),), dtype=torch.float64, device=dev)
	winv[:GP._winv.numel()] = GP._winv
	z = torch.zeros((cap,), dtype=torch.float64, device=dev)
	z[:n0] = GP._z[:n0]
	GP._factor = None
	torch.cuda.empty_cache()
	rows = torch.empty((kmax, n0 + kmax), dtype=torch.float64, device=dev)
	GP.kernel_object._kernel_into(x[:n0 + kmax], x[n0:].contiguous(), rows)
	rows[:, n0:] += 0.09 * torch.eye(kmax, dtype=torch.float64, device=dev)
	yn = y[n0:].reshape(-1).contiguous()
	info = torch.zeros((1,), dtype=torch.int32, device=dev)
	work = torch.empty((int(lib.stpy_potrf_append_workspace_bytes(0, n0, kmax)),), dtype=torch.uint8, device=dev)

	def refill(k):
		return lambda: A[n0:n0 + k, :n0 + k].copy_(rows[:k, :n0 + k])

	def append(k):
		return lambda: L.check(lib.stpy_potrf_append(0, n0, k, L.ptr(A), cap, L.ptr(winv), winv.numel(), L.ptr(z), L.ptr(yn), L.ptr(work),
													  work.numel(), L.ptr(info), L.stream_ptr()), "stpy_potrf_append")
	ys, zo = torch.zeros((n0,), dtype=torch.float64, device=dev), torch.empty((n0,), dtype=torch.float64, device=dev)
	trsv_ms = ev_time(lambda: L.check(lib.stpy_trsv(0, n0, L.ptr(A), cap, L.ptr(winv), winv.numel(), L.ptr(ys), L.ptr(zo), 0, L.stream_ptr()), "trsv"))
	res = {"n0": n0, "d": d, "dtype": "float64", "refit_ms": round(fit_ms, 1), "trsv_ms": round(trsv_ms, 3), "append_ms": {}}
	for k in (1, 4, 16, 64, 256):
		ms = ev_time(append(k), before=refill(k))
		assert int(info.item()) == 0
		res["append_ms"][k] = round(ms, 3)
		print("append k=%3d: %8.3f ms   (%.1fx one trsv, refit / append = %.0fx)" % (k, ms, ms / trsv_ms, fit_ms / ms), flush=True)
	old = lib.stpy_tune_get(34)
	cross = {}
	for k in (8, 16, 24, 32, 48, 64, 96, 128):
		lib.stpy_tune(34, 1 << 20)
		flow = ev_time(append(k), reps=3, before=refill(k))
		lib.stpy_tune(34, 0)
		mfma = ev_time(append(k), reps=3, before=refill(k))
		cross[k] = (round(flow, 3), round(mfma, 3))
		print("k=%3d  dataflow %8.3f ms   MFMA block solve %8.3f ms" % (k, flow, mfma), flush=True)
	lib.stpy_tune(34, old)
	res["crossover_flow_vs_mfma_ms"] = cross
	res["mfma_above_default"] = old
	L.check_async("append_bench")
	del A, winv, rows, work, GP
	torch.cuda.empty_cache()

	# ---- the optimisation loop at N0 = 16 384
	m0, iters = 16384, 128
	xl = torch.rand(m0 + iters, d, generator=g, dtype=torch.float64).to(dev)
	yl = torch.randn(m0 + iters, 1, generator=g, dtype=torch.float64).to(dev)
	cand = torch.rand(4096, d, generator=g, dtype=torch.float64).to(dev)
	loop = {}
	for mode in ("iterative", "refit"):
		G = GaussianProcess(gamma=1.0, s=0.3, kernel_name="squared_exponential", d=d)
		G.fit_gp(xl[:m0], yl[:m0])
		torch.cuda.synchronize()
		t = time.perf_counter()
		for i in range(iters):
			G.add_data_point(xl[m0 + i:m0 + i + 1], yl[m0 + i:m0 + i + 1], iterative=(mode == "iterative"))
			mu, sd = G.mean_std(cand)
		torch.cuda.synchronize()
		loop[mode] = round((time.perf_counter() - t) * 1e3 / iters, 2)
		print("N0=16384 loop (add 1 point + mean_std on 4096), %s: %.2f ms / iteration" % (mode, loop[mode]), flush=True)
	res["loop16k_ms_per_iter"] = loop
	print(json.dumps(res))


if __name__ == "__main__":
	main()
