"""Rank-k Cholesky update (stpy_chol_update) and the Thompson-sampling step of KernelizedFeatures on the MI355X.
For m = 4096, 8192, 16 384 features, fp64 and fp32, k = 1, 4, 16, 64, 128 new rows:
  (a) the stpy_chol_update call alone (device events, median after a warm-up call; the factor and W are restored untimed in front of
      each call), its bytes (one read and one write of the lower triangle per pass over L) per second, and a device fill of m^2
      elements for comparison;
  (b) one Thompson step -- add_data_point(k rows, iterative=True) + mean_std on 4096 candidates + sample_theta -- host clock around
      work that ends in a device synchronise, median over steps after a warm-up step;
  (c) the same step with iterative=False (the refit path), in the same run.
usage: python tools/kf_update_bench.py [m ...]      (default 4096 8192 16384)"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from stpy_amd import RFFEmbedding, _lib as L                                              # noqa: E402
from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures          # noqa: E402

KS = (1, 4, 16, 64, 128)
D, ROWS, CAND, STEPS = 8, 2048, 4096, 3
PASS_COLUMNS = 32          # columns of W per pass over L (csrc/cholupdate.hip: CU_KC)


def ev_time(fn, reps=5, before=None):
	"""median device time (ms) of fn over reps runs after one warm-up run; before() runs untimed in front of each"""
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


def model(emb, x, y, dtype):
	KF = KernelizedFeatures(embedding=emb, m=emb.get_m(), s=0.1, lam=1.0, d=D)
	KF.fit_gp(x[:ROWS].to(dtype), y[:ROWS].to(dtype))
	return KF


def thompson_ms(KF, x, y, cand, k, iterative, dtype):
	"""median wall time (ms) of STEPS steps after one warm-up step"""
	ts, r = [], ROWS
	for _ in range(STEPS + 1):
		torch.cuda.synchronize()
		t = time.perf_counter()
		KF.add_data_point(x[r:r + k].to(dtype), y[r:r + k].to(dtype), iterative=iterative)
		KF.mean_std(cand)
		KF.sample_theta()
		torch.cuda.synchronize()
		ts.append((time.perf_counter() - t) * 1e3)
		r += k
	return float(np.median(ts[1:]))


def main():
	ms_list = [int(a) for a in sys.argv[1:]] or [4096, 8192, 16384]
	dev = torch.device("cuda:0")
	lib = L.load()
	g = torch.Generator().manual_seed(1)
	total = ROWS + (STEPS + 1) * max(KS)
	x = (2 * torch.rand(total, D, generator=g, dtype=torch.float64) - 1).to(dev)
	y = torch.randn(total, 1, generator=g, dtype=torch.float64).to(dev)
	cand64 = (2 * torch.rand(CAND, D, generator=g, dtype=torch.float64) - 1).to(dev)
	res = {"library": lib.stpy_version().decode(), "rows": ROWS, "candidates": CAND, "configs": []}
	print("library:", res["library"], flush=True)
	for m in ms_list:
		np.random.seed(3)
		emb = RFFEmbedding(gamma=1.0, m=m, d=D)
		for dtype in (torch.float64, torch.float32):
			esz = 8 if dtype == torch.float64 else 4
			cand = cand64.to(dtype)
			KF = model(emb, x, y, dtype)
			L0, winv = KF._L.clone(), KF._winv.clone()
			W0 = emb.embed_t(x[ROWS:ROWS + max(KS)].to(dtype)).contiguous()          # (m, 128)
			Lw = torch.empty_like(L0)
			fill_ms = ev_time(lambda: Lw.zero_())
			row = {"m": m, "dtype": "float64" if esz == 8 else "float32", "fill_ms": round(fill_ms, 4),
				   "fill_GBps": round(m * m * esz / fill_ms / 1e6, 1), "k": {}}
			for k in KS:
				Wk = torch.empty((m, k), dtype=dtype, device=dev)
				work = torch.empty((max(int(lib.stpy_chol_update_workspace_bytes(L.dtype_code(dtype), m, k)), 1),), dtype=torch.uint8, device=dev)
				info = torch.zeros((1,), dtype=torch.int32, device=dev)

				def restore():
					Lw.copy_(L0)
					Wk.copy_(W0[:, :k])

				def call():
					L.check(lib.stpy_chol_update(L.dtype_code(dtype), m, k, 1, L.ptr(Lw), m, L.ptr(winv), winv.numel(), L.ptr(Wk), k, L.ptr(work), work.numel(),
												 L.ptr(info), L.stream_ptr()), "stpy_chol_update")
				a_ms = ev_time(call, before=restore)
				assert int(info.item()) == 0
				passes = -(-k // PASS_COLUMNS)
				a_gbps = passes * m * m * esz / a_ms / 1e6
				b_ms = thompson_ms(model(emb, x, y, dtype), x, y, cand, k, True, dtype)
				c_ms = thompson_ms(model(emb, x, y, dtype), x, y, cand, k, False, dtype)
				row["k"][k] = {"update_ms": round(a_ms, 3), "update_GBps": round(a_gbps, 1), "step_iterative_ms": round(b_ms, 2), "step_refit_ms": round(c_ms, 2)}
				print("m=%5d %s k=%3d  (a) update %8.3f ms = %7.1f GB/s (fill %.1f GB/s)   (b) step, iterative %8.2f ms   (c) step, refit %8.2f ms" % (
					m, row["dtype"], k, a_ms, a_gbps, row["fill_GBps"], b_ms, c_ms), flush=True)
			res["configs"].append(row)
			del KF, L0, winv, W0, Lw
			torch.cuda.empty_cache()
	L.check_async("kf_update_bench")
	print(json.dumps(res))


if __name__ == "__main__":
	main()
