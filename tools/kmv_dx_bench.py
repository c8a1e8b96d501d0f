"""
Matrix-free input gradients and pathwise samples (stpy_kmv_dx, csrc/kmvdx.hip; IterativeGaussianProcess.sample_paths / sample_and_optimize) at
the sizes the route is for.

  dx      stpy_kmv_dx at the few-queries shape: n = 64 and 1024 query points against q = 262 144 and 1 048 576 contracted points, d = 8 and 16,
          t = 1 and 16 coefficient rows, fp64 and fp32, squared exponential, uniform(-1, 1) data.  Beside it, in the same run and on the same
          operands: stpy_kmv (values only: the floor, 1 instead of d + 1 matrix instructions per pair); stpy_kmv_dtheta at the same pair
          count (square, sqrt(n q) points, t pairs of rows: the sibling with the same instruction mix per pair); and t calls of
          stpy_gram_grad, the only route to the same gradients without the new kernel (one coefficient vector per call, no values).
  paths   end to end at N = 262 144, d = 8, fp64: fit_gp, then sample_paths(size = 16) split into basis + residual slabs and the block solve
          (the solve is timed around ``_solve``, which ends in a host read), then the climbing of sample_and_optimize(size = 16, multistart = 32)
          on those paths (its own sample_paths would repeat the same draw and solve: its time is the sum of the two); beside the climbing, ONE mean_std block solve of 64 test points, the price an
          acquisition by variance pays per 64 candidates.

Each dx timing is a pair of device events around the call(s), after one warm-up of the same shape; reported are the median and the spread
(max - min) / median of the repetitions.  The paths part is host clocks around work that ends in a device synchronise, one run each.
Prints ONE JSON line on stdout; the table goes to stderr as it is measured.
usage: python tools/kmv_dx_bench.py [--part dx,paths] [--reps 5] [--n-paths 262144] [--quick]
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


def bench_dx(ns, qs, reps, dev):
	rows = []
	for dtype in (torch.float64, torch.float32):
		name = "f64" if dtype == torch.float64 else "f32"
		for q in qs:
			for d in (8, 16):
				b = points(q, d, dtype, dev)
				inv_ls = torch.full((d,), 1.0 / GAMMA[d], dtype=dtype, device=dev)
				for n in ns:
					a = points(n, d, dtype, dev, seed=1)
					nsq = int(round(np.sqrt(float(n) * q)))
					xs = points(nsq, d, dtype, dev, seed=2)
					for t in (1, 16):
						Vt = torch.from_numpy(np.random.RandomState(t).standard_normal((t, q))).to(device=dev, dtype=dtype)
						out = torch.empty((t, n, d + 1), dtype=dtype, device=dev)
						wx = _lib.kmv_dx_workspace(n, q, d, t, out)
						Yt = torch.empty((t, n), dtype=dtype, device=dev)
						wk = _lib.kmv_workspace(n, q, d, t, Yt)
						Us = torch.from_numpy(np.random.RandomState(t + 1).standard_normal((t, nsq))).to(device=dev, dtype=dtype)
						od = torch.empty((t, d + 2), dtype=dtype, device=dev)
						wd = _lib.kmv_dtheta_workspace(nsq, d, t, od)
						G = torch.empty((n, d), dtype=dtype, device=dev)

						def gg():
							for c in range(t):
								_lib.gram_grad(_lib.K_SE, b, a, G, inv_ls, alpha=Vt[c])
						row = {"dtype": name, "n": n, "q": q, "d": d, "t": t, "pairs": n * q, "dtheta_points": nsq,
							   "kmv_dx": timed(lambda: _lib.kmv_dx(_lib.K_SE, a, b, Vt, out, inv_ls, work=wx), reps),
							   "kmv": timed(lambda: _lib.kmv(_lib.K_SE, a, b, Vt, Yt, inv_ls, work=wk), reps),
							   "kmv_dtheta": timed(lambda: _lib.kmv_dtheta(_lib.K_SE, xs, inv_ls, Us, Us, od, work=wd), reps),
							   "gram_grad_t_calls": timed(gg, reps)}
						# the last gram_grad call left the gradient of row t - 1: the two routes agree
						row["max_abs_diff_vs_gram_grad"] = float((out[t - 1, :, :d] - G).abs().max().item())
						row["max_abs_diff_vs_kmv"] = float((out[:, :, d] - Yt).abs().max().item())
						row["Gpairs_per_s"] = round(n * q / (row["kmv_dx"]["median_ms"] * 1e-3) / 1e9, 2)
						rows.append(row)
						print("%s n=%5d q=%8d d=%2d t=%2d  kmv_dx %9.3f ms (+-%4.1f%%) %7.2f Gpair/s | kmv %9.3f | kmv_dtheta(%d^2) %9.3f | %2d x gram_grad %9.3f ms | "
							  "max |diff| grad %.1e value %.1e" % (name, n, q, d, t, row["kmv_dx"]["median_ms"], 100 * row["kmv_dx"]["spread"], row["Gpairs_per_s"],
							  row["kmv"]["median_ms"], nsq, row["kmv_dtheta"]["median_ms"], t, row["gram_grad_t_calls"]["median_ms"],
							  row["max_abs_diff_vs_gram_grad"], row["max_abs_diff_vs_kmv"]), file=sys.stderr, flush=True)
						del Vt, out, wx, Yt, wk, Us, od, wd, G
					del a, xs
				del b
	return rows


def clock(fn):
	torch.cuda.synchronize()
	t0 = time.time()
	r = fn()
	torch.cuda.synchronize()
	return r, time.time() - t0


def bench_paths(n, d, size, multistart, features, dev):
	rng = np.random.RandomState(n % 1000 + d)
	x = torch.from_numpy(rng.uniform(-1, 1, size=(n, d))).to(dev)
	y = torch.sin(3 * x[:, :1]) + 0.1 * torch.from_numpy(rng.normal(size=(n, 1))).to(dev)
	k = stpy_amd.KernelFunction(kernel_name="squared_exponential", gamma=GAMMA[d], d=d)
	gp = stpy_amd.IterativeGaussianProcess(kernel=k, s=0.1, precond_rank=256, maxiter=3000)
	torch.cuda.reset_peak_memory_stats()
	_, t_fit = clock(lambda: gp.fit_gp(x, y))
	out = {"what": "IterativeGaussianProcess, fp64, SE, s = 0.1, tol 1e-8, rank-256 preconditioner", "n": n, "d": d, "size": size, "multistart": multistart,
		   "features": features, "fit_s": round(t_fit, 3), "fit_info": dict(gp.cg_info)}
	print("fit n=%d d=%d: %.2f s, %s" % (n, d, t_fit, out["fit_info"]), file=sys.stderr, flush=True)
	solve_s = [0.0]
	inner = gp._solve

	def solve_timed(*a, **kw):
		r, dt = clock(lambda: inner(*a, **kw))
		solve_s[0] += dt
		return r
	gp._solve = solve_timed
	paths, t_paths = clock(lambda: gp.sample_paths(size=size, num_features=features, seed=1))
	out["sample_paths_s"] = round(t_paths, 3)
	out["sample_paths_solve_s"] = round(solve_s[0], 3)
	out["sample_paths_basis_residual_s"] = round(t_paths - solve_s[0], 3)
	out["path_info"] = dict(gp.path_info)
	print("sample_paths(size=%d, m=%d): %.2f s = basis + residual slabs %.2f s + block solve %.2f s, %s" % (
		size, features, t_paths, t_paths - solve_s[0], solve_s[0], out["path_info"]), file=sys.stderr, flush=True)
	xt = torch.from_numpy(rng.uniform(-1, 1, size=(size * multistart, d))).to(dev)
	which = torch.arange(size, device=dev).repeat_interleave(multistart)
	paths._value_grad_device(xt, which)
	out["one_stacked_evaluation"] = stats(event_ms(lambda: paths._value_grad_device(xt, which), 5))
	# the climbing alone: sample_and_optimize with the SAME seed would draw and solve the same paths again, so it is handed the ones above
	inner_paths = gp.sample_paths
	gp.sample_paths = lambda *a, **kw: paths
	np.random.seed(3)
	(sol, vals), t_climb = clock(lambda: gp.sample_and_optimize(size=size, multistart=multistart, num_features=features, seed=1))
	gp.sample_paths, gp._solve = inner_paths, inner
	out["climbing_s"] = round(t_climb, 3)
	out["sample_and_optimize_s"] = round(t_paths + t_climb, 3)
	out["climbing_evaluations"] = int(gp.optimize_info["evaluations"])
	out["best_values"] = [round(float(v), 4) for v in vals.cpu().numpy()]
	print("sample_and_optimize(size=%d, multistart=%d): sample_paths %.2f s + climbing %.2f s in %d stacked evaluations of %d points (one evaluation %.3f ms)" % (
		size, multistart, t_paths, t_climb, out["climbing_evaluations"], size * multistart, out["one_stacked_evaluation"]["median_ms"]), file=sys.stderr, flush=True)
	launches = gp.cg_info["kmv_launches"]
	_, t_ms = clock(lambda: gp.mean_std(xt[:64]))
	out["mean_std_64_points_s"] = round(t_ms, 3)
	out["mean_std_64_points_kmv_launches"] = int(gp.cg_info["kmv_launches"] - launches)
	out["peak_device_GB"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
	print("mean_std(64 points): %.2f s, %d stpy_kmv launches; peak device memory %.2f GB" % (t_ms, out["mean_std_64_points_kmv_launches"], out["peak_device_GB"]),
		  file=sys.stderr, flush=True)
	return out


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--part", default="dx,paths")
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--n-paths", type=int, default=262144, help="N of the paths part")
	ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the whole tool")
	a = ap.parse_args()
	if not torch.cuda.is_available():
		print(json.dumps({"tool": "kmv_dx_bench", "error": "no GPU: nothing measured"}))
		return 1
	dev = _lib.device()
	parts = a.part.split(",")
	out = {"tool": "kmv_dx_bench", "library": _lib.load().stpy_version().decode(), "gamma": GAMMA}
	if "dx" in parts:
		out["dx"] = bench_dx((64,) if a.quick else (64, 1024), (4096,) if a.quick else (262144, 1048576), max(a.reps, 1), dev)
	if "paths" in parts:
		out["paths"] = bench_paths(2048 if a.quick else a.n_paths, 8, 4 if a.quick else 16, 4 if a.quick else 32, 256 if a.quick else 2048, dev)
	print(json.dumps(out))
	return 0


if __name__ == "__main__":
	sys.exit(main())
