"""
Pivoted partial Cholesky (stpy_pchol, csrc/pchol.hip) at the sizes the Nystrom route is for:

  n in {65 536, 262 144, 1 048 576} x m in {512, 2048}, fp64 and fp32, squared exponential, d = 4, gamma = 0.2, uniform(-1, 1) data.

The kernel is a streaming read: step j reads j rows of Ft, a run of rank r reads esz * n * r (r - 1) / 2 bytes.  Each timing is a pair of
device events around the one call (m + 2 launches, no host synchronisation inside), after a warm-up of the same shape; reported are the
median and the spread (max - min) / median of the repetitions, the algorithmic bytes over the median, and that rate as a fraction of a
streaming read measured IN THE SAME RUN on the same buffer: stpy_predict (the library's own HBM-bound row kernel, every element read
once) over Ft's m * n elements viewed as rows of 16 384, so that the read fills the chip at every shape; timed the same way.
At n = 65 536, for context only: GaussianProcess.fit_gp on the same points (the exact route: the full n x n Gram matrix and its
factorisation).
Prints ONE JSON line on stdout; the table goes to stderr as it is measured.
usage: python tools/pchol_bench.py [--reps 5] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stpy_amd                                    # noqa: E402
from stpy_amd import _lib                          # noqa: E402

D, GAMMA = 4, 0.2


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
	return {"median_ms": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 4)}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--quick", action="store_true", help="n = 65 536 and m = 512 only, no exact-GP context: a rehearsal of the whole tool")
	a = ap.parse_args()
	if not torch.cuda.is_available():
		print(json.dumps({"tool": "pchol_bench", "error": "no GPU: nothing measured"}))
		return 1
	reps = max(a.reps, 5)
	dev = _lib.device()
	ns = (65536,) if a.quick else (65536, 262144, 1048576)
	ms_ = (512,) if a.quick else (512, 2048)
	rows = []
	for dtype in (torch.float64, torch.float32):
		esz = 8 if dtype == torch.float64 else 4
		for n in ns:
			x = torch.from_numpy(np.random.RandomState(n % 1000).uniform(-1, 1, size=(n, D))).to(device=dev, dtype=dtype)
			inv_ls = torch.full((D,), 1.0 / GAMMA, dtype=dtype, device=dev)
			for m in ms_:
				keep = {}

				def run():
					keep["out"] = _lib.pchol(_lib.K_SE, x, inv_ls, m)
				run()                                                     # warm-up of the same shape
				torch.cuda.synchronize()
				t = stats(event_ms(run, reps))
				piv, Ft, dres, rank = keep["out"]
				r = int(rank.item())
				nbytes = esz * n * r * (r - 1) // 2
				Fv = Ft.reshape(-1, 16384)                               # (a view: Ft is contiguous and n a multiple of 16 384)
				assert Fv.data_ptr() == Ft.data_ptr()
				ones, mu = torch.ones((16384,), dtype=dtype, device=dev), torch.empty((Fv.shape[0],), dtype=dtype, device=dev)

				def stream():
					_lib.predict(Fv, ones, mu)
				stream()
				torch.cuda.synchronize()
				s = stats(event_ms(stream, reps))
				rate = nbytes / (t["median_ms"] * 1e-3) / 1e12
				srate = esz * n * m / (s["median_ms"] * 1e-3) / 1e12
				rows.append({"dtype": "f64" if esz == 8 else "f32", "n": n, "m": m, "rank": r, "pchol": t, "algorithmic_TB": round(nbytes / 1e12, 4),
							 "TB_per_s": round(rate, 3), "stream_read": s, "stream_buffer_GB": round(esz * n * m / 1e9, 3), "stream_TB_per_s": round(srate, 3),
							 "fraction_of_stream": round(rate / srate, 3), "trace_error": float(dres.double().sum().item())})
				print("%s n=%8d m=%5d rank %5d  pchol %10.2f ms (+-%4.1f%%)  %7.3f TB -> %6.3f TB/s | stream read of %7.3f GB: %8.3f ms (+-%4.1f%%) %6.3f TB/s | fraction %5.3f" % (
					rows[-1]["dtype"], n, m, r, t["median_ms"], 100 * t["spread"], nbytes / 1e12, rate, esz * n * m / 1e9, s["median_ms"], 100 * s["spread"], srate,
					rate / srate), file=sys.stderr, flush=True)
				del keep, piv, Ft, Fv, dres, rank, ones, mu
			del x
	context = None
	if not a.quick:
		n = 65536
		rng = np.random.RandomState(n % 1000)
		x = torch.from_numpy(rng.uniform(-1, 1, size=(n, D))).to(dev)
		y = torch.sin(3 * x[:, :1]) + 0.1 * torch.from_numpy(rng.normal(size=(n, 1))).to(dev)
		k = stpy_amd.KernelFunction(kernel_name="squared_exponential", gamma=GAMMA, d=D)
		gp = stpy_amd.GaussianProcess(s=0.1, kernel=k)
		gp.fit_gp(x, y)
		torch.cuda.synchronize()
		context = {"what": "GaussianProcess.fit_gp, fp64, same points", "n": n, **stats(event_ms(lambda: gp.fit_gp(x, y), reps))}
		print("context: exact GaussianProcess.fit_gp n=%d fp64 %10.2f ms (+-%4.1f%%)" % (n, context["median_ms"], 100 * context["spread"]), file=sys.stderr, flush=True)
	print(json.dumps({"tool": "pchol_bench", "library": _lib.load().stpy_version().decode(), "d": D, "gamma": GAMMA, "reps": reps, "cases": rows,
					  "exact_gp_context": context}))
	return 0


if __name__ == "__main__":
	sys.exit(main())
