"""
The stochastic evidence of IterativeGaussianProcess (stpy_kmv_dtheta, csrc/kmvgrad.hip; stpy_pcg_lanczos; log_marginal_estimate) at the
sizes the route is for.

  dtheta    stpy_kmv_dtheta at n = 65 536 and 262 144, d = 4 and 16, t = 17 pairs, fp64 and fp32, squared exponential, uniform(-1, 1) data, beside
            stpy_kmv at the same n, d and t = 17 in the same run.  The ratio of the two is the figure of merit: the derivative pass in units
            of the product every CG iteration pays.
  estimate  one IterativeGaussianProcess.log_marginal_estimate with its gradient (gamma and the noise) at N = 32 768, d = 16, SE, fp64, 16 probes,
            rank-256 preconditioner, beside GaussianProcess.log_marginal with its gradient on the same points.
  big       one log_marginal_estimate with gradient at N = 262 144 (no exact route: the dense factor would take 550 GB), timed once.

Each timing is a pair of device events around the call(s), after one warm-up of the same shape; reported are the median and the spread
(max - min) / median of the repetitions.  Prints ONE JSON line on stdout; the table goes to stderr as it is measured.
usage: python tools/slq_bench.py [--part dtheta,estimate,big] [--reps 5] [--sizes 65536,262144] [--quick]
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
T_PAIRS = 17


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


def bench_dtheta(ns, reps, dev):
	rows = []
	for dtype in (torch.float64, torch.float32):
		name = "f64" if dtype == torch.float64 else "f32"
		for n in ns:
			for d in (4, 16):
				x = points(n, d, dtype, dev)
				inv_ls = torch.full((d,), 1.0 / GAMMA[d], dtype=dtype, device=dev)
				t = T_PAIRS
				Ut = torch.from_numpy(np.random.RandomState(t).standard_normal((t, n))).to(device=dev, dtype=dtype)
				Vt = torch.from_numpy(np.random.RandomState(t + 1).standard_normal((t, n))).to(device=dev, dtype=dtype)
				out = torch.empty((t, d + 2), dtype=dtype, device=dev)
				Yt = torch.empty((t, n), dtype=dtype, device=dev)
				wd, wk = _lib.kmv_dtheta_workspace(n, d, t, out), _lib.kmv_workspace(n, n, d, t, Yt)

				def run():
					_lib.kmv_dtheta(_lib.K_SE, x, inv_ls, Ut, Vt, out, work=wd)

				def product():
					_lib.kmv(_lib.K_SE, x, x, Vt, Yt, inv_ls, diag_add=0.01, work=wk)
				run()
				product()
				torch.cuda.synchronize()
				sd, sk = stats(event_ms(run, reps)), stats(event_ms(product, reps))
				value_diff = float(((Ut.double() * Yt.double()).sum(dim=1) - 0.01 * out[:, d + 1].double() - out[:, d].double()).abs().max().item())
				row = {"dtype": name, "n": n, "d": d, "t": t, "kmv_dtheta": sd, "kmv": sk, "ratio": round(sd["median_ms"] / sk["median_ms"], 3),
					   "Gevals_per_s": round(n * n * ((t + 15) // 16) / (sd["median_ms"] * 1e-3) / 1e9, 2), "max_abs_value_diff": value_diff}
				rows.append(row)
				print("%s n=%7d d=%2d t=%2d  kmv_dtheta %10.3f ms (+-%4.1f%%)  kmv %10.3f ms (+-%4.1f%%)  ratio %6.2f  (%7.2f Geval/s; value column against kmv %.2e)" % (
					name, n, d, t, sd["median_ms"], 100 * sd["spread"], sk["median_ms"], 100 * sk["spread"], row["ratio"], row["Gevals_per_s"], value_diff),
					file=sys.stderr, flush=True)
				del x, Ut, Vt, Yt, out, wd, wk
	return rows


def regression_data(n, d, dev):
	rng = np.random.RandomState(n % 1000 + d)
	x = torch.from_numpy(rng.uniform(-1, 1, size=(n, d))).to(dev)
	y = torch.sin(3 * x[:, :1]) + 0.1 * torch.from_numpy(rng.normal(size=(n, 1))).to(dev)
	return x, y


def bench_estimate(n, d, reps, dev, exact):
	x, y = regression_data(n, d, dev)
	k = stpy_amd.KernelFunction(kernel_name="squared_exponential", gamma=GAMMA[d], d=d)
	gp = stpy_amd.IterativeGaussianProcess(kernel=k, s=0.1, precond_rank=256, maxiter=3000, num_probes=16)
	gp.x, gp.y = x, y
	keep = {}

	def value_and_gradient(est, method):
		g = torch.tensor([GAMMA[d]], dtype=torch.float64, requires_grad=True)
		est.s = torch.tensor([0.1], dtype=torch.float64, requires_grad=True)
		f = method(est.kernel_object, {"0": {"gamma": g}}, 1.0)
		f.backward()
		keep[type(est).__name__] = (float(f.detach().reshape(-1)[0]), float(g.grad[0]), float(est.s.grad.reshape(-1)[0]))

	def run():
		value_and_gradient(gp, gp.log_marginal_estimate)
	torch.cuda.reset_peak_memory_stats()
	t0 = time.time()
	run()
	torch.cuda.synchronize()
	first = time.time() - t0
	info = {key: (val if not isinstance(val, np.ndarray) else None) for key, val in gp.evidence_info.items() if key not in ("q", "grad_stderr")}
	info["grad_stderr"] = {key: [float(v) for v in np.atleast_1d(val)] for key, val in gp.evidence_info["grad_stderr"].items()}
	out = {"what": "IterativeGaussianProcess.log_marginal_estimate with gradient (gamma, s), fp64, SE, 16 probes, rank 256", "n": n, "d": d,
		   "first_call_s": round(first, 3), "evidence_info": info, "value_dgamma_ds": keep["IterativeGaussianProcess"],
		   "peak_device_GB": round(torch.cuda.max_memory_allocated() / 1e9, 3), "dense_matrix_GB": round(8 * n * n / 1e9, 1)}
	if reps > 0:
		out.update(stats(event_ms(run, reps)))
	print("estimate n=%d d=%d: first call %.2f s, value %.3f +- %.3f, gradient %s +- %s, %d iterations, %d launches, peak %.2f GB%s" % (
		n, d, first, info["value"], info["stderr"], keep["IterativeGaussianProcess"][1:], info["grad_stderr"], info["iterations"], info["kmv_launches"],
		out["peak_device_GB"], "" if reps <= 0 else ", median %.1f ms (+-%.1f%%)" % (out["median_ms"], 100 * out["spread"])), file=sys.stderr, flush=True)
	if exact:
		ge = stpy_amd.GaussianProcess(s=0.1, kernel=k)
		ge.fit_gp(x, y)

		def run_exact():
			value_and_gradient(ge, ge.log_marginal)
		run_exact()
		torch.cuda.synchronize()
		out["exact_gp_context"] = {"what": "GaussianProcess.log_marginal with gradient, same points", **stats(event_ms(run_exact, max(reps, 1))),
								   "value_dgamma_ds": keep["GaussianProcess"]}
		print("context: exact GaussianProcess.log_marginal with gradient n=%d %10.2f ms (+-%4.1f%%): value %.3f, gradient %s" % (
			n, out["exact_gp_context"]["median_ms"], 100 * out["exact_gp_context"]["spread"], keep["GaussianProcess"][0], keep["GaussianProcess"][1:]),
			file=sys.stderr, flush=True)
	return out


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--part", default="dtheta,estimate,big")
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--sizes", default="65536,262144", help="n of the dtheta part")
	ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the whole tool")
	a = ap.parse_args()
	if not torch.cuda.is_available():
		print(json.dumps({"tool": "slq_bench", "error": "no GPU: nothing measured"}))
		return 1
	dev = _lib.device()
	parts = a.part.split(",")
	out = {"tool": "slq_bench", "library": _lib.load().stpy_version().decode(), "gamma": GAMMA}
	if "dtheta" in parts:
		out["dtheta"] = bench_dtheta((4096,) if a.quick else tuple(int(v) for v in a.sizes.split(",")), max(a.reps, 1), dev)
	if "estimate" in parts:
		out["estimate"] = bench_estimate(2048 if a.quick else 32768, 16, a.reps, dev, exact=True)
	if "big" in parts:
		out["big"] = bench_estimate(4096 if a.quick else 262144, 16, 0, dev, exact=False)
	print(json.dumps(out))
	return 0


if __name__ == "__main__":
	sys.exit(main())
