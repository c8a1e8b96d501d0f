"""
Matrix-free kernel product and solver (stpy_kmv / stpy_pcg, csrc/kmv.hip; IterativeGaussianProcess) at the sizes the route is for.

  kmv     stpy_kmv at n = q = 65 536 and 262 144, d = 4 and 16, t = 1 / 16 / 64, fp64 and fp32, squared exponential, uniform(-1, 1) data:
          ms and kernel evaluations (n q) per second.  Beside it at n = 65 536, in the same run, the only route to the same product without
          it: stpy_gram into an n x n buffer, then stpy_gemm_nt (both timed together; the buffer is 34 GB in fp64).
  fit     IterativeGaussianProcess.fit_gp + mean at N = 65 536, d = 16, SE, fp64, with its iterations and stpy_kmv launches; beside it
          GaussianProcess.fit_gp + mean on the same points, as context.
  big     one IterativeGaussianProcess fit + mean at N = 262 144 (the dense factor would take 550 GB), with the peak device memory.

Each timing is a pair of device events around the call(s), after one warm-up of the same shape; reported are the median and the spread
(max - min) / median of the repetitions.  Prints ONE JSON line on stdout; the table goes to stderr as it is measured.
usage: python tools/kmv_bench.py [--part kmv,fit,big] [--reps 5] [--fit-reps 5] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stpy_amd                                    # noqa: E402
from stpy_amd import _lib                          # noqa: E402

GAMMA = {4: 0.5, 16: 2.0}


def event_ms(fn, reps):
	out = []
	for _ in range(reps):
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		a.record()
		fn()
		b.record()
		b.synchronize()
		out.append(a.elapsed_time(b))
	return out


def stats(ms):
	med = float(np.median(ms))
	return {"median_ms": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 4), "reps": len(ms)}


def points(n, d, dtype, dev):
	return torch.from_numpy(np.random.RandomState(n % 1000 + d).uniform(-1, 1, size=(n, d))).to(device=dev, dtype=dtype)


def bench_kmv(ns, reps, dev):
	rows = []
	for dtype in (torch.float64, torch.float32):
		name = "f64" if dtype == torch.float64 else "f32"
		for n in ns:
			for d in (4, 16):
				x = points(n, d, dtype, dev)
				inv_ls = torch.full((d,), 1.0 / GAMMA[d], dtype=dtype, device=dev)
				for t in (1, 16, 64):
					Vt = torch.from_numpy(np.random.RandomState(t).standard_normal((t, n))).to(device=dev, dtype=dtype)
					Yt = torch.empty((t, n), dtype=dtype, device=dev)
					work = _lib.kmv_workspace(n, n, d, t, Yt)

					def run():
						_lib.kmv(_lib.K_SE, x, x, Vt, Yt, inv_ls, diag_add=0.01, work=work)
					run()
					torch.cuda.synchronize()
					s = stats(event_ms(run, reps))
					row = {"dtype": name, "n": n, "d": d, "t": t, "kmv": s, "Gevals_per_s": round(n * n / (s["median_ms"] * 1e-3) / 1e9, 2)}
					line = "%s n=%7d d=%2d t=%2d  kmv %10.3f ms (+-%4.1f%%) %8.2f Geval/s" % (name, n, d, t, s["median_ms"], 100 * s["spread"], row["Gevals_per_s"])
					if n <= 65536:
						K = torch.empty((n, n), dtype=dtype, device=dev)
						Yd = torch.empty((t, n), dtype=dtype, device=dev)
						gw = _lib.gram_workspace(n, n, d, K)

						def dense():
							_lib.gram(_lib.K_SE, x, x, K, inv_ls, diag_add=0.01, work=gw)
							_lib.gemm_nt(Vt, K, Yd)
						dense()
						torch.cuda.synchronize()
						row["gram_then_gemm"] = stats(event_ms(dense, reps))
						row["max_abs_diff"] = float((Yd - Yt).abs().max().item())
						line += " | gram + gemm_nt %10.3f ms (+-%4.1f%%), %5.1f GB buffer, max |diff| %.2e" % (
							row["gram_then_gemm"]["median_ms"], 100 * row["gram_then_gemm"]["spread"], K.numel() * K.element_size() / 1e9, row["max_abs_diff"])
						del K, Yd, gw
					rows.append(row)
					print(line, file=sys.stderr, flush=True)
					del Vt, Yt, work
				del x
	return rows


def regression_data(n, d, dev):
	rng = np.random.RandomState(n % 1000 + d)
	x = torch.from_numpy(rng.uniform(-1, 1, size=(n, d))).to(dev)
	y = torch.sin(3 * x[:, :1]) + 0.1 * torch.from_numpy(rng.normal(size=(n, 1))).to(dev)
	xt = torch.from_numpy(rng.uniform(-1, 1, size=(4096, d))).to(dev)
	return x, y, xt


def bench_fit(n, d, reps, dev, exact):
	x, y, xt = regression_data(n, d, dev)
	k = stpy_amd.KernelFunction(kernel_name="squared_exponential", gamma=GAMMA[d], d=d)
	gp = stpy_amd.IterativeGaussianProcess(kernel=k, s=0.1, precond_rank=256, maxiter=3000)
	keep = {}

	def run():
		gp.fit_gp(x, y)
		keep["mu"] = gp.mean(xt)
	torch.cuda.reset_peak_memory_stats()
	t0 = time.time()
	run()
	torch.cuda.synchronize()
	first = time.time() - t0
	out = {"what": "IterativeGaussianProcess.fit_gp + mean(4096 points), fp64, SE", "n": n, "d": d, "first_call_s": round(first, 3), "cg_info": dict(gp.cg_info),
		   "tol": 1e-8, "peak_device_GB": round(torch.cuda.max_memory_allocated() / 1e9, 3), "dense_matrix_GB": round(8 * n * n / 1e9, 1)}
	if reps > 0:
		out.update(stats(event_ms(run, reps)))
	print("iterative n=%d d=%d: first call %.2f s, %s, peak %.2f GB%s" % (n, d, first, out["cg_info"], out["peak_device_GB"],
		  "" if reps <= 0 else ", median %.1f ms (+-%.1f%%)" % (out["median_ms"], 100 * out["spread"])), file=sys.stderr, flush=True)
	if exact:
		ge = stpy_amd.GaussianProcess(s=0.1, kernel=k)

		def run_exact():
			ge.fit_gp(x, y)
			keep["mu_exact"] = ge.mean(xt)
		run_exact()
		torch.cuda.synchronize()
		out["exact_gp_context"] = {"what": "GaussianProcess.fit_gp + mean, same points", **stats(event_ms(run_exact, max(reps, 1)))}
		out["max_abs_mean_diff"] = float((keep["mu"] - keep["mu_exact"]).abs().max().item())
		print("context: exact GaussianProcess n=%d %10.2f ms (+-%4.1f%%); max |mean difference| %.2e" % (
			n, out["exact_gp_context"]["median_ms"], 100 * out["exact_gp_context"]["spread"], out["max_abs_mean_diff"]), file=sys.stderr, flush=True)
	return out


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--part", default="kmv,fit,big")
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--fit-reps", type=int, default=5)
	ap.add_argument("--sizes", default="65536,262144", help="n of the kmv part")
	ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the whole tool")
	a = ap.parse_args()
	if not torch.cuda.is_available():
		print(json.dumps({"tool": "kmv_bench", "error": "no GPU: nothing measured"}))
		return 1
	dev = _lib.device()
	parts = a.part.split(",")
	out = {"tool": "kmv_bench", "library": _lib.load().stpy_version().decode(), "gamma": GAMMA}
	if "kmv" in parts:
		out["kmv"] = bench_kmv((4096,) if a.quick else tuple(int(v) for v in a.sizes.split(",")), max(a.reps, 1), dev)
	if "fit" in parts:
		out["fit"] = bench_fit(4096 if a.quick else 65536, 16, a.fit_reps, dev, exact=True)
	if "big" in parts:
		out["big"] = bench_fit(8192 if a.quick else 262144, 16, 0, dev, exact=False)
	print(json.dumps(out))
	return 0


if __name__ == "__main__":
	sys.exit(main())
