"""Randomised parity sweep through the drop-in classes against the CPU oracle (checker only): random sizes (ragged, tiny, around the
128 / 512 / 1024 tile and panel edges), dimensions, kernel families and hyper-parameters; fit_gp + mean_std (+ full covariance) +
log_marginal + add_data_point, in fp64 with the 1e-8 bar of SURVEY.md section 8d scaled by the conditioning of the case.
One case in five of the translation-invariant families moves x and xt by a common integer offset round(10^U(0,3)) (at most 100 in fp32)
and is compared with the oracle on the UNSHIFTED points: the Gram kernels must not lose digits to where the data lies.
usage: python tools/fuzz_parity.py [cases] [seed] [rff cases]        exit code 1 on the first failure (the failing case is printed)"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from oracle import gp_oracle as O          # checker only
from stpy_amd import GaussianProcess, KernelFunction

import os
from stpy_amd import _lib as _L
for _kv in filter(None, os.environ.get("STPY_TUNE", "").split(",")):          # e.g. STPY_TUNE=29=2 with the lab library: A/B of a route under the same cases
	_L.load().stpy_tune(int(_kv.split("=")[0]), int(_kv.split("=")[1]))
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rng = np.random.RandomState(seed)
rng_off = np.random.RandomState(seed + 977)          # the offsets have a stream of their own: every older draw of a seed keeps its meaning
dev = torch.device("cuda:0")
SIZES = [1, 2, 3, 5, 17, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 383, 511, 512, 513, 640, 700, 1023, 1024, 1025, 1300, 2047, 2048, 2100, 3000]


def rel(a, b):
	nb = np.linalg.norm(b)
	return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


t_start = time.time()
worst = 0.0
n_f32 = 0
for case in range(cases):
	n = int(rng.choice(SIZES)) if rng.uniform() < 0.8 else int(rng.randint(1, 1500))
	d = int(rng.choice([1, 2, 3, 5, 8, 16, 17, 33]))
	m = int(rng.choice([1, 2, 7, 64, 129, 300, 1000]))
	fam = rng.choice(["squared_exponential", "ard", "matern", "ard_matern", "linear", "polynomial", "sum", "product"])
	s = float(10.0 ** rng.uniform(-2, 0))
	kappa = float(rng.uniform(0.5, 3.0))
	gamma = float(np.sqrt(d) * rng.uniform(0.5, 2.0))
	nu = float(rng.choice([0.5, 1.5, 2.5]))
	ardg = (np.sqrt(d) * rng.uniform(0.5, 2.0, size=d)).astype(np.float64)
	if d == 1:          # kernels.py:36-39: torch.Tensor([ard_gamma]) succeeds for a one-element tensor and rounds it to fp32 (the drop-in does the same)
		ardg = ardg.astype(np.float32).astype(np.float64)
	x = rng.uniform(-1, 1, size=(n, d))
	y = np.sin(x.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(n, 1))
	xt = rng.uniform(-1, 1, size=(m, d))
	if fam == "squared_exponential":
		ko = KernelFunction(kernel_name=fam, gamma=gamma, kappa=kappa, d=d); spec = [(fam, {"gamma": gamma, "kappa": kappa}, "-")]
	elif fam == "ard":
		ko = KernelFunction(kernel_name=fam, ard_gamma=torch.from_numpy(ardg), kappa=kappa, d=d); spec = [(fam, {"ard_gamma": ardg, "kappa": kappa}, "-")]
	elif fam == "matern":
		ko = KernelFunction(kernel_name=fam, gamma=gamma, nu=nu, kappa=kappa, d=d); spec = [(fam, {"gamma": gamma, "nu": nu, "kappa": kappa}, "-")]
	elif fam == "ard_matern":
		ko = KernelFunction(kernel_name=fam, ard_gamma=torch.from_numpy(ardg), nu=nu, kappa=kappa, d=d); spec = [(fam, {"ard_gamma": ardg, "nu": nu, "kappa": kappa}, "-")]
	elif fam == "linear":
		ko = KernelFunction(kernel_name=fam, kappa=kappa, d=d); spec = [(fam, {"kappa": kappa}, "-")]
	elif fam == "polynomial":
		ko = KernelFunction(kernel_name=fam, kappa=kappa, power=2, d=d); spec = [(fam, {"kappa": kappa, "degree": 2}, "-")]
	else:
		k1 = KernelFunction(kernel_name="squared_exponential", gamma=gamma, kappa=kappa, d=d)
		k2 = KernelFunction(kernel_name="matern", gamma=1.5 * gamma, nu=nu, kappa=1.0, d=d)
		ko = (k1 + k2) if fam == "sum" else (k1 * k2)
		spec = [("squared_exponential", {"gamma": gamma, "kappa": kappa}, "-"), ("matern", {"gamma": 1.5 * gamma, "nu": nu, "kappa": 1.0}, "+" if fam == "sum" else "*")]
	u_off, e_off = rng_off.uniform(), rng_off.uniform(0, 3)
	off = float(round(10.0 ** e_off)) if (u_off < 0.2 and fam not in ("linear", "polynomial")) else 0.0
	desc = "case %d: n=%d d=%d m=%d %s s=%.3g kappa=%.3g gamma=%.3g nu=%.1f" % (case, n, d, m, fam, s, kappa, gamma, nu)
	try:
		Ko = O.gram_train(x, spec, s)
		cond = np.linalg.cond(Ko) if n <= 1500 else 1e6
		tol = max(1e-8, 1e-13 * cond)
		# a quarter of the well-conditioned cases run in fp32 (BASELINE config 3's precision; bar 1e-3)
		f32 = bool(rng.uniform() < 0.5) and s >= 0.2 and cond < 5e3
		tdt = torch.float32 if f32 else torch.float64
		if f32:
			tol = max(1e-3, 1e-6 * cond)
		if off:
			# the device sees the shifted points rounded to its dtype; the oracle sees exactly those points moved back
			off = min(off, 100.0) if f32 else off
			ndt = np.float32 if f32 else np.float64
			x_dev, xt_dev = (x + off).astype(ndt).astype(np.float64), (xt + off).astype(ndt).astype(np.float64)
			x, xt = x_dev - off, xt_dev - off
			desc += " offset=%g" % off
		else:
			x_dev, xt_dev = x, xt
		L, alpha = O.fit(x, y, spec, s)
		mu_o, sd_o = O.mean_std(x, L, alpha, xt, spec)
		lml_o = float(O.log_marginal(x, y, spec, s)[0, 0])
		gp = GaussianProcess(kernel=ko, s=s, d=d)
		xd, yd, xtd = (torch.from_numpy(v).to(dev).to(tdt) for v in (x_dev, y, xt_dev))
		gp.fit_gp(xd, yd)
		mu, sd = gp.mean_std(xtd)
		lml = float(gp.log_marginal(gp.kernel_object, {}, 1.0).item())
		# (the mean's error is taken relative to the larger of |mu_o| and the data's rms scale over the same number of points: with one or two test
		# points a posterior mean that happens to be near zero would otherwise turn an absolute error at rounding level into a relative one of 1e-2
		# -- seed 406, case 84: fp32, m = 1, cond 3e3, 3.5e-3 against the bar of 3.1e-3 with one diagonal-block kernel and 2.4e-3 with the other)
		mu_scale = max(float(np.linalg.norm(mu_o)), float(np.sqrt(np.mean(y * y)) * np.sqrt(m)))
		e = [float(np.linalg.norm(mu.cpu().numpy() - mu_o)) / mu_scale, rel(sd.cpu().numpy(), sd_o), abs(lml - lml_o) / max(1.0, abs(lml_o))]
		# the posterior std cancels (k** - ...): its error scales with kappa / sigma_min
		sd_floor = float(np.abs(sd_o).min())
		tol_sd = tol * max(1.0, kappa / max(sd_floor, 1e-300)) if sd_floor > 0 else np.inf
		assert mu.shape == (m, 1) and sd.shape == (m, 1), (mu.shape, sd.shape)
		assert e[0] < tol and e[1] < tol_sd and e[2] < tol, (e, tol, tol_sd)
		if m <= 129:
			mu2, cov = gp.mean_std(xtd, full=True)
			_, cov_o = O.mean_cov(x, L, alpha, xt, spec)
			assert rel(cov.cpu().numpy(), cov_o) < max(tol, tol_sd), ("full covariance", rel(cov.cpu().numpy(), cov_o))
		if case % 5 == 0 and n >= 2:          # incremental data: drop the last point, fit, add it back (gauss_procc.py:100-111)
			gp2 = GaussianProcess(kernel=ko, s=s, d=d)
			gp2.fit_gp(xd[:-1], yd[:-1])
			gp2.add_data_point(xd[-1:], yd[-1:])
			mu3, sd3 = gp2.mean_std(xtd)
			assert rel(mu3.cpu().numpy(), mu_o) < tol and rel(sd3.cpu().numpy(), sd_o) < tol_sd, ("add_data_point", rel(mu3.cpu().numpy(), mu_o))
		worst = max(worst, e[0] / tol, e[2] / tol)
		n_f32 += int(f32)
	except Exception as ex:          # noqa: BLE001
		print("FAILED", desc, "->", type(ex).__name__, ex, flush=True)
		sys.exit(1)
	if case % 20 == 0:
		print("ok", desc, "fp32" if f32 else "fp64", "cond %.1e  err mu %.1e sd %.1e lml %.1e" % (cond, e[0], e[1], e[2]), flush=True)
print("all %d cases passed in %.0f s (%d of them in fp32); worst error / tolerance %.2f" % (cases, time.time() - t_start, n_f32, worst))

# ---- RFF embed (embedding.py:225-241): every route of stpy_rff_embed is reached by some shape below -- the bf16-split streaming kernel
# (fp32, d = 64, n >= 8192, m % 1024 == 0), the tile kernels (d = 32 / 64, n % 128 == 0, m % 64 == 0), the GEMM epilogue (everything
# else), the fp64 GEMM + trig pass; plain and biased (the biased form comes back transposed, as in the reference)
from stpy_amd import RFFEmbedding
rcases = max(cases // 4, 8) if len(sys.argv) < 4 else int(sys.argv[3])
for case in range(rcases):
	dt = torch.float64 if rng.uniform() < 0.5 else torch.float32
	n = int(rng.choice([1, 3, 33, 127, 128, 129, 640, 1000, 4096, 8192, 8192 + 384]))
	d = int(rng.choice([1, 2, 5, 17, 32, 64]))
	mm = int(rng.choice([2, 6, 64, 130, 192, 1024, 2048, 3072]))
	biased = bool(rng.uniform() < 0.3)
	gam = float(np.sqrt(d) * rng.uniform(0.7, 3.0))
	kap = float(rng.uniform(0.5, 2.0))
	desc = "rff case %d: %s n=%d d=%d m=%d biased=%s gamma=%.3g" % (case, str(dt)[6:], n, d, mm, biased, gam)
	try:
		emb = RFFEmbedding(gamma=gam, m=mm, d=d, kappa=kap, biased=biased)
		emb.W = torch.from_numpy(rng.normal(size=(mm, d)) / gam)
		if biased:
			emb.b = torch.from_numpy(2 * np.pi * rng.uniform(size=mm))
		xx = rng.uniform(-1, 1, size=(n, d))
		xq = xx.astype(np.float32 if dt == torch.float32 else np.float64)
		Wq = emb.W.numpy().astype(np.float32 if dt == torch.float32 else np.float64).astype(np.float64)
		bq = None if not biased else emb.b.numpy().astype(np.float32 if dt == torch.float32 else np.float64).astype(np.float64)
		z = emb.embed(torch.from_numpy(xq).to(dev)).cpu().numpy()
		ref = O.rff_embed(xq.astype(np.float64), Wq, mm, kappa=kap, b=bq)
		assert z.shape == ref.shape, (z.shape, ref.shape)
		amp = np.sqrt(2.0 / mm) * np.sqrt(kap)
		phase = float(np.abs(xq.astype(np.float64) @ Wq.T).max()) + (2 * np.pi if biased else 0.0)
		tol = amp * (1e-13 * max(1.0, phase) if dt == torch.float64 else max(2e-5, 6e-6 * phase))
		err = float(np.abs(z - ref).max())
		assert err < tol, (err, tol)
	except Exception as ex:          # noqa: BLE001
		print("FAILED", desc, "->", type(ex).__name__, ex, flush=True)
		sys.exit(1)
	if case % 10 == 0:
		print("ok", desc, "err / amplitude %.1e" % (err / amp), flush=True)
print("all %d rff cases passed" % rcases)
