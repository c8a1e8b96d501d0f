"""
Local experts: what a fit, an evidence gradient and a prediction cost (DESIGN.md "Local experts").

  kernels     stpy_experts_fit with and without a gradient at n_e = 256, E = 1024, d = 8, per expert, beside stpy_lml_batch at n = 256,
              batch = 1024, d = 8 per candidate -- from this build and, with --parent-lib (repeatable), from other builds of libstpy_hip.so
              (the parent commit's), all alternating inside one process; "ratios" then holds, per entry point, this build over the first
              parent and, with two parents, the per-round range of one parent over the other: the noise a ratio has to be read against;
              stpy_experts_predict + stpy_experts_combine at M = 4096
  end to end  LocalExpertsGaussianProcess at N = 1 048 576, d = 8, expert_size = 256: fit_gp, one log_marginal with its gradient, mean_std of
              4096 points; workspace and factor bytes at that size
  gradients   on that committee: stpy_experts_predict_grad + stpy_experts_combine_grad beside stpy_experts_predict + stpy_experts_combine on the
              same chunks of test points at M = 256 and M = 4096 (device events, the ratio per round), mean_std_grad beside mean_std (host
              clocks; the gradient path has its own, smaller chunks), and one ucb_optimize(multistart=256) with its evaluation count

Kernel times are device events around `--reps` back-to-back launches after a warm-up, median and spread over `--rounds` rounds; end-to-end times
are host clocks around calls that end in a read-back or a synchronise.  Prints one JSON line.

usage: python tools/experts_bench.py [--reps 5] [--rounds 5] [--parent-lib PATH]... [--n 256] [--d 8] [--kernels-only] [--no-grad] [--quick]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stpy_amd import _lib  # noqa: E402


def _events(fn, reps):
	a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	a.record()
	for _ in range(reps):
		fn()
	b.record()
	b.synchronize()
	return a.elapsed_time(b) / reps


def _stats(v):
	v = np.asarray(v)
	return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def _lml_batch_call(lib, x, y, inv_ls, noise, pidx, kappa=1.0):
	"""a closure that launches stpy_lml_batch of the library handle ``lib`` (this build's or another's) on fixed buffers"""
	lib.stpy_lml_batch_workspace_bytes.restype, lib.stpy_lml_batch_workspace_bytes.argtypes = _lib.SIGNATURES["stpy_lml_batch_workspace_bytes"]
	lib.stpy_lml_batch.restype, lib.stpy_lml_batch.argtypes = _lib.SIGNATURES["stpy_lml_batch"]
	n, d, B = x.shape[0], x.shape[1], inv_ls.shape[0]
	value = torch.empty(B, dtype=torch.float64, device=x.device)
	grad = torch.empty((B, 2), dtype=torch.float64, device=x.device)
	info = torch.empty(B, dtype=torch.int32, device=x.device)
	work = torch.empty(int(lib.stpy_lml_batch_workspace_bytes(0, n, d, B)), dtype=torch.uint8, device=x.device)
	keep = (value, grad, info, work)

	def call():
		rc = lib.stpy_lml_batch(0, 0, _lib.ptr(x), n, d, d, None, _lib.ptr(y), B, _lib.ptr(inv_ls), d, _lib.ptr(noise), kappa, 1.0, _lib.ptr(pidx), 1,
								_lib.ptr(value), _lib.ptr(grad), 2, _lib.ptr(info), _lib.ptr(work), work.numel(), _lib.stream_ptr())
		assert rc == 0, rc
	call.keep = keep
	return call


def _experts_fit_call(lib, xs, ys, offsets, n_e, inv_ls, noise, pidx, factor, alpha, work, with_grad, kappa=1.0):
	"""the same for stpy_experts_fit, with or without a gradient (one lengthscale slot); factor / alpha / work are shared between the variants"""
	lib.stpy_experts_fit.restype, lib.stpy_experts_fit.argtypes = _lib.SIGNATURES["stpy_experts_fit"]
	N, d, E = xs.shape[0], xs.shape[1], offsets.numel() - 1
	value = torch.empty(E, dtype=torch.float64, device=xs.device)
	grad = torch.empty((E, 2), dtype=torch.float64, device=xs.device) if with_grad else None
	total = torch.empty(3, dtype=torch.float64, device=xs.device)
	info = torch.empty(E, dtype=torch.int32, device=xs.device)

	def call():
		rc = lib.stpy_experts_fit(0, 0, _lib.ptr(xs), N, d, d, None, _lib.ptr(ys), _lib.ptr(offsets), E, n_e, _lib.ptr(inv_ls), _lib.ptr(noise), kappa, 1.0,
								  _lib.ptr(pidx) if with_grad else None, 1 if with_grad else 0, _lib.ptr(factor), factor.numel(), _lib.ptr(alpha), _lib.ptr(value),
								  _lib.ptr(grad), 2 if with_grad else 0, _lib.ptr(total), _lib.ptr(info), _lib.ptr(work), work.numel(), _lib.stream_ptr())
		assert rc == 0, rc
		return info
	call.keep = (value, grad, total, info)
	return call


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--rounds", type=int, default=5)
	ap.add_argument("--parent-lib", action="append", default=[])
	ap.add_argument("--n", type=int, default=256, help="points per expert and per candidate")
	ap.add_argument("--d", type=int, default=8)
	ap.add_argument("--kernels-only", action="store_true")
	ap.add_argument("--quick", action="store_true")
	ap.add_argument("--no-grad", action="store_true", help="skip the input-gradient section (prediction with and without gradients, ucb_optimize)")
	a = ap.parse_args()
	if not torch.cuda.is_available():
		print(json.dumps({"tool": "experts_bench", "error": "no GPU: nothing measured"}))
		return 1
	dev = _lib.device()
	lib = _lib.load()
	gen = torch.Generator(device="cpu").manual_seed(0)
	n_e, E, d, M = a.n, (64 if a.quick else 1024), a.d, (256 if a.quick else 4096)
	ls, s = 0.8, 0.1
	out = {"tool": "experts_bench", "library": lib.stpy_version().decode(), "n_e": n_e, "E": E, "d": d, "M": M, "reps": a.reps, "rounds": a.rounds}

	# ---- kernels: E different blocks under one candidate / E candidates on one block
	xs = torch.rand((E * n_e, d), generator=gen, dtype=torch.float64).to(dev)
	ys = (torch.sin(3 * xs[:, 0]) + 0.1 * torch.randn(E * n_e, generator=gen, dtype=torch.float64).to(dev)).contiguous()
	offsets = torch.arange(0, (E + 1) * n_e, n_e, dtype=torch.int32, device=dev)
	inv_ls = torch.full((d,), 1.0 / ls, dtype=torch.float64, device=dev)
	noise = torch.tensor([s], dtype=torch.float64, device=dev)
	pidx = torch.zeros(d, dtype=torch.int32, device=dev)
	factor = _lib.experts_factor(n_e, E, xs)
	alpha = torch.empty(E * n_e, dtype=torch.float64, device=dev)
	work = _lib.experts_fit_workspace(n_e, d, E, xs)
	inv_b = inv_ls.reshape(1, d).repeat(E, 1).contiguous()
	noise_b = noise.repeat(E).contiguous()
	entries = ("experts_fit_grad", "experts_fit", "lml_batch")
	suffixes = [""] + ["_parent" if i == 0 else "_parent%d" % (i + 1) for i in range(len(a.parent_lib))]
	runs = {}
	for sfx, handle in zip(suffixes, [lib] + [ctypes.CDLL(os.path.abspath(path)) for path in a.parent_lib]):
		runs["experts_fit_grad" + sfx] = _experts_fit_call(handle, xs, ys, offsets, n_e, inv_ls, noise, pidx, factor, alpha, work, True)
		runs["experts_fit" + sfx] = _experts_fit_call(handle, xs, ys, offsets, n_e, inv_ls, noise, pidx, factor, alpha, work, False)
		runs["lml_batch" + sfx] = _lml_batch_call(handle, xs[:n_e], ys[:n_e], inv_b, noise_b, pidx)
	info = runs["experts_fit"]()
	xt = torch.rand((M, d), generator=gen, dtype=torch.float64).to(dev)
	mu_e = torch.empty((E, M), dtype=torch.float64, device=dev)
	var_e = torch.empty((E, M), dtype=torch.float64, device=dev)
	mu, var = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
	chunk = max(32, min(M, (1 << 20) // E))
	pwork = _lib._work(lib.stpy_experts_predict_workspace_bytes(0, n_e, d, E, chunk), xs)

	def predict_combine():
		for c in range(0, M, chunk):
			_lib.experts_predict(0, xs, offsets, n_e, inv_ls, 1.0, factor, alpha, info, xt[c:c + chunk], mu_e[:, c:c + chunk], var_e[:, c:c + chunk], work=pwork)
		_lib.experts_combine(3, mu_e, var_e, 1.0, mu, var)
	runs["predict_combine"] = predict_combine
	times = {k: [] for k in runs}
	for k, fn in runs.items():          # warm-up: code objects, allocations
		fn()
	torch.cuda.synchronize()
	fits = [k for k in runs if k != "predict_combine"]
	for r in range(a.rounds):          # alternating, so that a drift of the box hits every variant alike, and each round starting one variant later, so
		for k in fits[r % len(fits):] + fits[:r % len(fits)]:          # that no variant always runs behind the same neighbour
			times[k].append(_events(runs[k], a.reps))
		runs["experts_fit"]()          # (the prediction reads this build's factor and alpha)
		times["predict_combine"].append(_events(predict_combine, a.reps))
	assert int(info.any().item()) == 0
	out["kernels"] = {k: dict(_stats(v), per_expert_us=float(np.median(v)) * 1e3 / E) for k, v in times.items()}
	if a.parent_lib:          # per round: this build over the first parent; with a second parent, parent over parent2 (what equal code measures)
		ratio = lambda p, q: [float(x / y) for x, y in zip(times[p], times[q])]
		out["ratios"] = {}
		for k in entries:
			r = ratio(k, k + "_parent")
			out["ratios"][k] = {"new_over_parent_median": float(np.median(r)), "new_over_parent_min": min(r), "new_over_parent_max": max(r)}
			if len(a.parent_lib) > 1:
				pp = ratio(k + "_parent", k + "_parent2")
				out["ratios"][k].update(parent_over_parent2_min=min(pp), parent_over_parent2_max=max(pp), parent_over_parent2_median=float(np.median(pp)))
	out["predict_chunk"] = chunk
	out["bytes_at_E"] = {"factor": factor.numel(), "fit_workspace": work.numel(), "predict_workspace": pwork.numel()}
	del factor, alpha, work, pwork, mu_e, var_e, runs
	torch.cuda.empty_cache()
	if a.kernels_only:
		print(json.dumps(out))
		return 0

	# ---- end to end
	import stpy_amd
	N = (1 << 14) if a.quick else (1 << 20)
	x = torch.rand((N, d), generator=gen, dtype=torch.float64)
	y = (torch.sin(3 * x[:, :1]) * torch.cos(2 * x[:, 1:2]) + 0.1 * torch.randn((N, 1), generator=gen, dtype=torch.float64))
	xd, yd, xtd = x.to(dev), y.to(dev), xt
	gp = stpy_amd.LocalExpertsGaussianProcess(gamma=ls, s=s, d=d, expert_size=n_e)
	e2e = {"fit_gp": [], "evidence_grad": [], "mean_std": []}
	for r in range(1 + max(a.rounds, 1)):          # (round 0 warms up)
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		gp.fit_gp(xd, yd)
		torch.cuda.synchronize()
		t1 = time.perf_counter()
		g = torch.tensor([ls], dtype=torch.float64, requires_grad=True)
		f = gp.log_marginal(gp.kernel_object, {'0': {'gamma': g, 'kappa': 1.0, 'group': list(range(d))}}, 1.0)
		f.backward()
		torch.cuda.synchronize()
		t2 = time.perf_counter()
		m_, s_ = gp.mean_std(xtd)
		torch.cuda.synchronize()
		t3 = time.perf_counter()
		if r > 0:
			e2e["fit_gp"].append((t1 - t0) * 1e3)
			e2e["evidence_grad"].append((t2 - t1) * 1e3)
			e2e["mean_std"].append((t3 - t2) * 1e3)
	Ebig = gp.experts_info["E"]
	out["end_to_end"] = dict({k: _stats(v) for k, v in e2e.items()}, N=N, E=Ebig, M=M, evidence=float(f.detach()), dgamma=float(g.grad), predict_chunk=gp._chunks(M)[0][1],
							 factor_bytes=gp.experts_info["factor_bytes"], fit_workspace_bytes=int(lib.stpy_experts_fit_workspace_bytes(0, n_e, d, Ebig)),
							 predict_workspace_bytes=int(lib.stpy_experts_predict_workspace_bytes(0, n_e, d, Ebig, gp._chunks(M)[0][1])))
	if a.no_grad:
		print(json.dumps(out))
		return 0

	# ---- input gradients on the fitted committee: stpy_experts_predict_grad + _combine_grad beside stpy_experts_predict + _combine on the SAME chunks
	# (the prediction's), device events; then the class (its own chunk rule for the gradient path), host clocks; then one ucb_optimize
	kind, kappa, cols, il, nmax = gp._hyper
	out["gradients"] = {}
	for Mk in sorted({min(256, M), M}):
		xk = xtd[:Mk]
		chunks = gp._chunks(Mk)
		cm = max(b - c for c, b in chunks)
		z = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
		mu_e, var_e, gmu_e, gvar_e = z(Ebig, cm), z(Ebig, cm), z(Ebig, cm, d), z(Ebig, cm, d)
		mu, var, dmu, dstd = z(Mk), z(Mk), z(Mk, d), z(Mk, d)
		pw = _lib._work(lib.stpy_experts_predict_workspace_bytes(0, nmax, d, Ebig, cm), xd)
		gw = _lib.experts_predict_grad_workspace(nmax, d, Ebig, cm, xd)

		def plain():
			for c, b in chunks:
				_lib.experts_predict(kind, gp._xs, gp._offsets, nmax, il, kappa, gp._factor, gp._alpha, gp._info, xk[c:b], mu_e[:, :b - c], var_e[:, :b - c], cols=cols, work=pw)
				_lib.experts_combine(3, mu_e[:, :b - c], var_e[:, :b - c], kappa, mu[c:b], var[c:b])

		def grad():
			for c, b in chunks:
				_lib.experts_predict_grad(kind, gp._xs, gp._offsets, nmax, il, kappa, gp._factor, gp._alpha, gp._info, xk[c:b], mu_e[:, :b - c], var_e[:, :b - c],
										  gmu_e[:, :b - c], gvar_e[:, :b - c], cols=cols, work=gw)
				_lib.experts_combine_grad(3, mu_e[:, :b - c], var_e[:, :b - c], gmu_e[:, :b - c], gvar_e[:, :b - c], kappa, mu[c:b], var[c:b], dmu[c:b], dstd[c:b])
		tk = {"predict_combine": [], "predict_grad_combine_grad": [], "mean_std": [], "mean_std_grad": []}
		plain(), grad(), gp.mean_std(xk), gp.mean_std_grad(xk)          # warm-up
		torch.cuda.synchronize()
		for r in range(max(a.rounds, 1)):
			tk["predict_combine"].append(_events(plain, a.reps))
			tk["predict_grad_combine_grad"].append(_events(grad, a.reps))
			for name, fn in (("mean_std", gp.mean_std), ("mean_std_grad", gp.mean_std_grad)):
				torch.cuda.synchronize()
				t0 = time.perf_counter()
				fn(xk)
				torch.cuda.synchronize()
				tk[name].append((time.perf_counter() - t0) * 1e3)
		ratio = [g_ / p_ for g_, p_ in zip(tk["predict_grad_combine_grad"], tk["predict_combine"])]
		out["gradients"]["M=%d" % Mk] = dict({k: _stats(v) for k, v in tk.items()}, chunk=cm, grad_chunk=gp._grad_chunks(Mk, d)[0][1],
											 grad_over_plain_median=float(np.median(ratio)), grad_over_plain_min=min(ratio), grad_over_plain_max=max(ratio),
											 grad_workspace_bytes=gw.numel(), plain_workspace_bytes=pw.numel())
		del mu_e, var_e, gmu_e, gvar_e, pw, gw
		torch.cuda.empty_cache()
	print(json.dumps({"gradients_so_far": out["gradients"]}), file=sys.stderr, flush=True)
	gp.bounds = [(0.0, 1.0)] * d
	np.random.seed(0)
	starts = 16 if a.quick else 256
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	sol, val = gp.ucb_optimize(4.0, multistart=starts)
	torch.cuda.synchronize()
	out["ucb_optimize"] = {"multistart": starts, "ms": (time.perf_counter() - t0) * 1e3, "evaluations": gp.optimize_info["evaluations"],
						   "launches": gp.optimize_info["launches"], "value": float(val), "best_start_value": float(gp.optimize_info["start_values"].max())}
	print(json.dumps(out))
	return 0


if __name__ == "__main__":
	sys.exit(main())
