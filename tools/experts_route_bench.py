"""
Local experts: what the k-d partition and routed prediction cost and buy (DESIGN.md "Local experts: spatial partition and routed prediction").

The committee of tools/experts_bench.py -- N = 1 048 576, d = 8, experts of 256 (E = 4096), SE kernel -- in ONE process:
  fit         fit_gp with partition="random" beside partition="kdtree"; the k-d partition alone (scaled coordinates, the levels, the read-back
              of the order) is timed separately
  prediction  on the k-d committee, unrouted (predict_experts=None: the all-experts path, code routing does not touch) beside routed with
              k = 1, 4, 8, alternating per round: mean_std of 4096 and of 256 points, mean_std_grad of 256 and of 4096 points, and one
              ucb_optimize(multistart=256) each; per configuration the launches and, for the routed ones, the tiles a launch really uses beside
              the host-side bound
  accuracy    RMSE against the noiseless function on 4096 held-out points: "kdtree" with all experts, with k = 1, 4, 8, and "random" with all
              experts and with k = 4

Times are host clocks around calls that end in a read-back or a synchronise, after one warm-up round per shape; median and spread over
--rounds rounds of one call (unrouted) or --routed-reps back-to-back calls (routed: a call is about a millisecond), per call.  Prints one JSON line.

usage: python tools/experts_route_bench.py [--rounds 3] [--routed-reps 20] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stpy_amd import _lib  # noqa: E402


def _stats(v):
	v = np.asarray(v)
	return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def _clock(fn):
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	out = fn()
	torch.cuda.synchronize()
	return (time.perf_counter() - t0) * 1e3, out


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--rounds", type=int, default=3)
	ap.add_argument("--routed-reps", type=int, default=20, help="calls per timed window of a routed configuration (the unrouted ones take one)")
	ap.add_argument("--quick", action="store_true", help="N = 16 384 and 256 test points: a rehearsal of the script, not a measurement")
	a = ap.parse_args()
	if not torch.cuda.is_available():
		print(json.dumps({"tool": "experts_route_bench", "error": "no GPU: nothing measured"}))
		return 1
	import stpy_amd
	dev = _lib.device()
	gen = torch.Generator(device="cpu").manual_seed(0)
	n_e, d, ls, s = 256, 8, 0.8, 0.1
	N, M, starts = ((1 << 14), 256, 16) if a.quick else ((1 << 20), 4096, 256)
	f = lambda x: torch.sin(3 * x[:, :1]) * torch.cos(2 * x[:, 1:2])
	x = torch.rand((N, d), generator=gen, dtype=torch.float64)
	y = f(x) + s * torch.randn((N, 1), generator=gen, dtype=torch.float64)
	xt = torch.rand((M, d), generator=gen, dtype=torch.float64)
	xd, yd, xtd, truth = x.to(dev), y.to(dev), xt.to(dev), f(xt).numpy().ravel()
	out = {"tool": "experts_route_bench", "library": _lib.load().stpy_version().decode(), "N": N, "d": d, "expert_size": n_e, "M": M, "rounds": a.rounds, "routed_reps": a.routed_reps}
	make = lambda part, k: stpy_amd.LocalExpertsGaussianProcess(gamma=ls, s=s, d=d, expert_size=n_e, partition=part, predict_experts=k, bounds=[(0.0, 1.0)] * d)

	# ---- fit: random beside kdtree, alternating; the partition alone
	fit = {"random": [], "kdtree": [], "kdtree_partition_alone": []}
	gps = {"random": make("random", None), "kdtree": make("kdtree", None)}
	for r in range(1 + a.rounds):          # (round 0 warms up)
		for part, gp in gps.items():
			t, _ = _clock(lambda: gp.fit_gp(xd, yd))
			if r:
				fit[part].append(t)
		t, _ = _clock(lambda: gps["kdtree"]._partition(N, xd))
		if r:
			fit["kdtree_partition_alone"].append(t)
	out["fit_gp"] = dict({k: _stats(v) for k, v in fit.items()}, E=gps["kdtree"].experts_info["E"])
	rmse = lambda gp: float(np.sqrt(np.mean((gp.mean(xtd).cpu().numpy().ravel() - truth) ** 2)))
	out["rmse"] = {"random_all": rmse(gps["random"]), "kdtree_all": rmse(gps["kdtree"])}
	rk = make("random", 4)
	rk.fit_gp(xd, yd)
	out["rmse"]["random_k4"] = rmse(rk)
	del rk, gps["random"]
	torch.cuda.empty_cache()

	# ---- prediction: unrouted beside k = 1, 4, 8 on the k-d committee
	configs = {"all": gps["kdtree"]}
	for k in (1, 4, 8):
		configs["k%d" % k] = make("kdtree", k)
		configs["k%d" % k].fit_gp(xd, yd)
		out["rmse"]["kdtree_k%d" % k] = rmse(configs["k%d" % k])
	E = configs["all"].experts_info["E"]
	shapes = [("mean_std_%d" % M, "mean_std", M), ("mean_std_256", "mean_std", 256), ("mean_std_grad_256", "mean_std_grad", 256), ("mean_std_grad_%d" % M, "mean_std_grad", M)]
	times = {name: {key: [] for key, _, _ in shapes} for name in configs}
	pred = {name: {} for name in configs}
	for r in range(1 + a.rounds):
		for name, gp in configs.items():
			for key, method, m in shapes:
				before = gp.launches
				reps = 1 if gp.predict_experts is None else a.routed_reps          # (a routed call is a millisecond: a window of several)
				t, _ = _clock(lambda: [getattr(gp, method)(xtd[:m]) for _ in range(reps)])
				if r:
					times[name][key].append(t / reps)
				pred[name][key + "_launches"] = (gp.launches - before) // reps
	for name, gp in configs.items():
		pred[name].update({key: _stats(v) for key, v in times[name].items()})
		if gp.predict_experts is not None:          # the tiles a launch of all M points uses, beside the bound it is launched with
			wexp, _ = _lib.experts_work_list(gp._route_device(xtd), E)
			pred[name].update(tiles_used=int((wexp >= 0).sum().item()), tiles_bound=int(wexp.numel()), tiles_unrouted=E * (-(-M // 32)))
		np.random.seed(0)
		t, (sol, val) = _clock(lambda: gp.ucb_optimize(4.0, multistart=starts))
		pred[name]["ucb_optimize"] = {"multistart": starts, "ms": t, "evaluations": gp.optimize_info["evaluations"], "launches": gp.optimize_info["launches"],
									  "value": float(val), "best_start_value": float(gp.optimize_info["start_values"].max())}
	out["prediction"] = pred
	base = pred["all"]
	out["speedup_over_all"] = {name: {key: base[key]["median_ms"] / pred[name][key]["median_ms"] for key, _, _ in shapes} for name in configs if name != "all"}
	print(json.dumps(out))
	return 0


if __name__ == "__main__":
	sys.exit(main())
