"""
Matrix-free second-order and standard-deviation input derivatives (stpy_kmv_dxx, csrc/kmvdxx.hip; IterativeGaussianProcess.ucb_optimize) at the
sizes the route is for.

  dxx     stpy_kmv_dxx at the few-queries shape: n = 64 query points against q = 1 048 576 contracted points, d = 8 and 16, t = 1 and 16
          coefficient rows, fp64 and fp32, squared exponential, uniform(-1, 1) data.  Beside it, in the same run and on the same operands,
          stpy_kmv_dx.  The matrix-instruction count predicts a ratio of (1 + d + d (d + 1) / 2) / (1 + d): 5 at d = 8, 9 at d = 16; the
          measured ratio is reported beside it (nothing is gated on it).
  ucb     end to end at N = 65 536, d = 8, fp64: fit_gp, then ONE ucb_optimize(multistart = 64) with its evaluation and solve counts, and the
          time per evaluation beside the time of the fit (the expectation: about one fit per evaluation at rhs_block = 64).

Each dxx timing is a pair of device events around the call, after one warm-up of the same shape; reported are the median and the spread
(max - min) / median of the repetitions.  The ucb part is host clocks around work that ends in a device synchronise, one run each.
Prints ONE JSON line on stdout; the table goes to stderr as it is measured.
usage: python tools/kmv_dxx_bench.py [--part dxx,ucb] [--reps 5] [--n-ucb 65536] [--quick]
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

GAMMA = {8: 1.0, 16: 2.0}


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


def timed(fn, reps):
	fn()
	torch.cuda.synchronize()
	return stats(event_ms(fn, reps))


def points(n, d, dtype, dev, seed=0):
	return torch.from_numpy(np.random.RandomState(n % 1000 + d + seed).uniform(-1, 1, size=(n, d))).to(device=dev, dtype=dtype)


def bench_dxx(n, q, reps, dev):
	rows = []
	for dtype in (torch.float64, torch.float32):
		name = "f64" if dtype == torch.float64 else "f32"
		for d in (8, 16):
			b = points(q, d, dtype, dev)
			a = points(n, d, dtype, dev, seed=1)
			inv_ls = torch.full((d,), 1.0 / GAMMA[d], dtype=dtype, device=dev)
			nc = _lib.kmv_dxx_ncol(d)
			for t in (1, 16):
				Vt = torch.from_numpy(np.random.RandomState(t).standard_normal((t, q))).to(device=dev, dtype=dtype)
				out2 = torch.empty((t, n, nc), dtype=dtype, device=dev)
				w2 = _lib.kmv_dxx_workspace(n, q, d, t, out2)
				out1 = torch.empty((t, n, d + 1), dtype=dtype, device=dev)
				w1 = _lib.kmv_dx_workspace(n, q, d, t, out1)
				row = {"dtype": name, "n": n, "q": q, "d": d, "t": t, "pairs": n * q, "columns": nc,
					   "kmv_dxx": timed(lambda: _lib.kmv_dxx(_lib.K_SE, a, b, Vt, out2, inv_ls, work=w2), reps),
					   "kmv_dx": timed(lambda: _lib.kmv_dx(_lib.K_SE, a, b, Vt, out1, inv_ls, work=w1), reps)}
				row["ratio"] = round(row["kmv_dxx"]["median_ms"] / row["kmv_dx"]["median_ms"], 2)
				row["predicted_ratio"] = round(nc / (d + 1.0), 2)
				row["max_abs_diff_first_block_vs_kmv_dx"] = float((out2[:, :, :d + 1] - out1).abs().max().item())
				row["Gpairs_per_s"] = round(n * q / (row["kmv_dxx"]["median_ms"] * 1e-3) / 1e9, 2)
				rows.append(row)
				print("%s n=%d q=%d d=%2d t=%2d  kmv_dxx %9.3f ms (+-%4.1f%%) %7.2f Gpair/s | kmv_dx %9.3f ms (+-%4.1f%%) | ratio %5.2f (instruction count: %4.2f) | "
					  "max |diff| first block %.1e" % (name, n, q, d, t, row["kmv_dxx"]["median_ms"], 100 * row["kmv_dxx"]["spread"], row["Gpairs_per_s"],
					  row["kmv_dx"]["median_ms"], 100 * row["kmv_dx"]["spread"], row["ratio"], row["predicted_ratio"], row["max_abs_diff_first_block_vs_kmv_dx"]),
					  file=sys.stderr, flush=True)
				del Vt, out1, out2, w1, w2
			del a, b
	return rows


def clock(fn):
	torch.cuda.synchronize()
	t0 = time.time()
	r = fn()
	torch.cuda.synchronize()
	return r, time.time() - t0


def bench_ucb(n, d, multistart, dev):
	rng = np.random.RandomState(n % 1000 + d)
	x = torch.from_numpy(rng.uniform(-1, 1, size=(n, d))).to(dev)
	y = torch.sin(3 * x[:, :1]) + 0.1 * torch.from_numpy(rng.normal(size=(n, 1))).to(dev)
	k = stpy_amd.KernelFunction(kernel_name="squared_exponential", gamma=GAMMA[d], d=d)
	gp = stpy_amd.IterativeGaussianProcess(kernel=k, s=0.1, precond_rank=256, maxiter=3000, rhs_block=64, bounds=[(-1.0, 1.0)] * d)
	torch.cuda.reset_peak_memory_stats()
	_, t_fit = clock(lambda: gp.fit_gp(x, y))
	out = {"what": "IterativeGaussianProcess, fp64, SE, s = 0.1, tol 1e-8, rank-256 preconditioner, rhs_block 64", "n": n, "d": d, "multistart": multistart,
		   "fit_s": round(t_fit, 3), "fit_info": dict(gp.cg_info)}
	print("fit n=%d d=%d: %.2f s, %s" % (n, d, t_fit, out["fit_info"]), file=sys.stderr, flush=True)
	np.random.seed(3)
	(sol, val), t_opt = clock(lambda: gp.ucb_optimize(4.0, multistart=multistart))
	info = gp.optimize_info
	out.update({"ucb_optimize_s": round(t_opt, 3), "evaluations": int(info["evaluations"]), "solves": int(info["solves"]), "kmv_launches": int(info["kmv_launches"]),
				"s_per_evaluation": round(t_opt / info["evaluations"], 3), "evaluation_over_fit": round(t_opt / info["evaluations"] / t_fit, 2),
				"value": round(float(val), 6), "best_start_value": round(float(info["start_values"].max()), 6),
				"peak_device_GB": round(torch.cuda.max_memory_allocated() / 1e9, 3)})
	print("ucb_optimize(multistart=%d): %.2f s in %d evaluations = %d block solves, %d stpy_kmv launches: %.2f s per evaluation = %.2f fits; value %.4f "
		  "(best start %.4f); peak device memory %.2f GB" % (multistart, t_opt, out["evaluations"], out["solves"], out["kmv_launches"], out["s_per_evaluation"],
		  out["evaluation_over_fit"], out["value"], out["best_start_value"], out["peak_device_GB"]), file=sys.stderr, flush=True)
	xt = torch.from_numpy(rng.uniform(-1, 1, size=(multistart, d))).to(dev)
	gp.mean_value_grad_hessian(xt)
	out["mean_value_grad_hessian_%d_points" % multistart] = stats(event_ms(lambda: gp.mean_value_grad_hessian(xt), 5))
	return out


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--part", default="dxx,ucb")
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--n-ucb", type=int, default=65536, help="N of the ucb part")
	ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the whole tool")
	a = ap.parse_args()
	if not torch.cuda.is_available():
		print(json.dumps({"tool": "kmv_dxx_bench", "error": "no GPU: nothing measured"}))
		return 1
	dev = _lib.device()
	parts = a.part.split(",")
	out = {"tool": "kmv_dxx_bench", "library": _lib.load().stpy_version().decode(), "gamma": GAMMA}
	if "dxx" in parts:
		out["dxx"] = bench_dxx(64, 4096 if a.quick else 1048576, max(a.reps, 1), dev)
	if "ucb" in parts:
		out["ucb"] = bench_ucb(2048 if a.quick else a.n_ucb, 8, 8 if a.quick else 64, dev)
	print(json.dumps(out))
	return 0


if __name__ == "__main__":
	sys.exit(main())
