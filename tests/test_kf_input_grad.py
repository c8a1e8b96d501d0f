"""
Input gradients of the feature-space posterior: stpy_rff_grad (csrc/rffgrad.hip), the embeddings' value_grad / derivative_1 /
derivative_2, and the KernelizedFeatures surface built on them (autograd through mean_std / mean_var / mean / ucb / lcb,
sample_and_optimize, the private Hessian helper).

The NumPy closed forms below are the checker: on the CPU they must reproduce the reference's autograd numbers in G18
(tests/golden/make_golden_kf_grad.py); on the GPU the device results must reproduce G18, and the C ABI is checked against an
fp64 torch evaluation of the same sums on the device.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.conftest import golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stpy_amd", "csrc")

# ---------------------------------------------------------------- the G18 models (same table as tests/golden/make_golden_kf_grad.py)
CASES = {
	"rff": ("RFFEmbedding", dict(gamma=0.8, m=32, d=3, kappa=1.5), 120, True),
	"hermite": ("HermiteEmbedding", dict(gamma=0.5, m=2 * 6 ** 2, d=2, kappa=1.2), 120, True),
	"dual": ("RFFEmbedding", dict(gamma=0.8, m=32, d=3, kappa=1.5), 20, False),
}


def make_embedding(case, g):
	import stpy_amd
	cls, kw, _, _ = CASES[case]
	emb = getattr(stpy_amd, cls)(**kw)
	if cls == "RFFEmbedding":
		emb.W = torch.from_numpy(g["rff_W"].copy())
	return emb


def make_model(case, g):
	from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures
	emb = make_embedding(case, g)
	KF = KernelizedFeatures(embedding=emb, m=emb.get_m(), s=float(g["s"]), lam=float(g["lam"]), d=CASES[case][1]["d"], primal=CASES[case][3])
	KF.fit_gp(torch.from_numpy(g[case + "_x"]), torch.from_numpy(g[case + "_y"]))
	return KF


# ---------------------------------------------------------------- closed forms (NumPy, fp64)

def np_operands(emb):
	"""(W, bias, feat_scale, scale) of the embedding's feature map from its HOST attributes (no device call)."""
	if hasattr(emb, "weights"):                                   # quadrature family: cos | sin of the same nodes, amplitudes sqrt(w_j)
		W = emb.W.numpy()
		amp = np.sqrt(emb.weights.numpy().reshape(-1))
		return np.concatenate([W, W]), None, np.concatenate([amp, amp]), np.sqrt(emb.kappa)
	bias = emb.b.numpy().reshape(-1) if emb.biased else None
	return emb.W.numpy(), bias, None, np.sqrt(2.0 / emb.m) * np.sqrt(emb.kappa)


def features(ops, x):
	"""Phi (n, m) and Phi' (n, m): the feature values and the derivative of each with respect to its own phase."""
	W, bias, fs, scale = ops
	q = x @ W[:, :x.shape[1]].T
	a = scale * (fs if fs is not None else np.ones(W.shape[0]))
	if bias is not None:
		return a * np.cos(q + bias), -a * np.sin(q + bias)
	h = W.shape[0] // 2
	phi = np.concatenate([np.cos(q[:, :h]), np.sin(q[:, h:])], axis=1)
	dphi = np.concatenate([-np.sin(q[:, :h]), np.cos(q[:, h:])], axis=1)
	return a * phi, a * dphi


def value_grad_hess(ops, x, C):
	"""val (n,), G (n, d), H (n, d, d) of sum_j C_tj phi_j(x_t); C: (n, m) or (m,)."""
	W = ops[0][:, :x.shape[1]]
	phi, dphi = features(ops, x)
	C = np.broadcast_to(C, phi.shape)
	return (C * phi).sum(1), (C * dphi) @ W, -np.einsum("tj,jk,jl->tkl", C * phi, W, W)


def posterior(ops, x, y, s, lam, primal):
	"""theta (m,) and Z (m, m): mu = phi^T theta, sigma^2 = phi^T Z phi."""
	Phi = features(ops, x)[0]
	n, m = Phi.shape
	if primal:
		Vinv = np.linalg.inv(Phi.T @ Phi + s * s * lam * np.eye(m))
		return Vinv @ (Phi.T @ y).reshape(-1), s * s * Vinv
	Kinv = np.linalg.inv(Phi @ Phi.T + s * s * lam * np.eye(n))
	return Phi.T @ (Kinv @ y).reshape(-1), (np.eye(m) - Phi.T @ Kinv @ Phi) / lam


def posterior_grads(ops, theta, Z, xt):
	"""mu, std (n,), d mu, d std (n, d), Hessian of mu (n, d, d)."""
	phi = features(ops, xt)[0]
	mu, dmu, hmu = value_grad_hess(ops, xt, theta)
	PZ = phi @ Z
	std = np.sqrt((PZ * phi).sum(1))
	_, dstd, _ = value_grad_hess(ops, xt, PZ / std[:, None])
	return mu, std, dmu, dstd, hmu


# ---------------------------------------------------------------- CPU: argument checks, closed forms against the reference, resources

def _lib():
	from stpy_amd import _lib as L
	return L


def _rg(lib, dtype=0, x=16, n=5, ldx=8, d=3, W=16, ldw=8, m=8, bias=None, C=16, ldc=8, order=1, combine=0, G=16, ldg=8, H=None, work=16,
		work_bytes=1 << 20):
	vp = lambda v: ctypes.c_void_p(v) if v else None
	return lib.stpy_rff_grad(dtype, vp(x), n, ldx, d, vp(W), ldw, m, vp(bias), None, 1.0, vp(C), ldc, order, combine, None, vp(G), ldg, vp(H),
							 vp(work), work_bytes, None)


def test_rff_grad_argument_checks():
	L = _lib()
	lib = L.load()
	assert _rg(lib, dtype=7) == -1
	assert b"dtype" in lib.stpy_last_error_string()
	assert _rg(lib, x=0) == -2
	assert _rg(lib, d=0) == -5
	assert _rg(lib, d=-2) == -5
	assert _rg(lib, ldx=2) == -4
	assert _rg(lib, W=0) == -6
	assert _rg(lib, ldw=2) == -7
	assert _rg(lib, m=7) == -8                                # odd m without a bias
	assert b"even" in lib.stpy_last_error_string()
	assert _rg(lib, m=7, bias=16, ldc=7, work=0) == -20       # ... is accepted with one (the next check fails)
	assert _rg(lib, C=0) == -12
	assert _rg(lib, ldc=5) == -13
	assert _rg(lib, ldc=0, work=0) == -20                     # ldc == 0: the shared row
	assert _rg(lib, order=0) == -14
	assert _rg(lib, order=3) == -14
	assert _rg(lib, combine=2) == -15                         # STPY_OUT_MUL
	assert _rg(lib, G=0) == -17
	assert _rg(lib, ldg=2) == -18
	assert _rg(lib, order=2, H=0) == -19
	assert _rg(lib, work=0) == -20
	assert _rg(lib, work_bytes=8) == -21
	assert b"workspace" in lib.stpy_last_error_string()
	# empty problems return 0 without looking at a pointer
	assert lib.stpy_rff_grad(7, None, 0, 0, 0, None, 0, 8, None, None, 1.0, None, 0, 5, 9, None, None, 0, None, None, 0, None) == 0
	assert lib.stpy_rff_grad(7, None, 5, 0, 0, None, 0, 0, None, None, 1.0, None, 0, 5, 9, None, None, 0, None, None, 0, None) == 0
	assert lib.stpy_rff_grad_workspace_bytes(0, 0, 3, 64, 1) == 0
	assert lib.stpy_rff_grad_workspace_bytes(0, 10, 3, 0, 1) == 0
	for order in (1, 2):
		q64 = lib.stpy_rff_grad_workspace_bytes(0, 25, 4, 32768, order)
		assert q64 > 0 and lib.stpy_rff_grad_workspace_bytes(1, 25, 4, 32768, order) * 2 == q64
	assert lib.stpy_rff_grad_workspace_bytes(0, 4096, 16, 8192, 2) > lib.stpy_rff_grad_workspace_bytes(0, 4096, 16, 8192, 1) > 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_closed_forms_reproduce_reference(case):
	g = golden("G18_kf_input_grad")
	ops = np_operands(make_embedding(case, g))
	theta, Z = posterior(ops, g[case + "_x"], g[case + "_y"], float(g["s"]), float(g["lam"]), CASES[case][3])
	assert rel_err(theta, g[case + "_theta"].reshape(-1)) < 1e-10
	assert rel_err(Z, g[case + "_Z"]) < 1e-10
	mu, std, dmu, dstd, _ = posterior_grads(ops, theta, Z, g[case + "_xb"])
	assert rel_err(mu, g[case + "_mu"].reshape(-1)) < 1e-10
	assert rel_err(std, g[case + "_std"].reshape(-1)) < 1e-10
	assert rel_err(dmu, g[case + "_dmu_sum"]) < 1e-10
	assert rel_err(dstd, g[case + "_dstd_sum"]) < 1e-10
	_, _, gm, _, hm = posterior_grads(ops, theta, Z, g[case + "_pts"])
	assert rel_err(gm, g[case + "_grad"]) < 1e-10
	assert rel_err(hm, g[case + "_hess"]) < 1e-10
	if case == "hermite":
		# the full Jacobians: z1[k, j, t] = d phi_j(x_t) / dx_k, z2[k, l, j, t] = d2 phi_j(x_t) / dx_k dx_l
		W = ops[0]
		phi, dphi = features(ops, g[case + "_xb"])
		assert rel_err(np.einsum("tj,jk->kjt", dphi, W), g[case + "_d1"]) < 1e-10
		assert rel_err(-np.einsum("tj,jk,jl->kljt", phi, W, W), g[case + "_d2"]) < 1e-10


RES_F64_REGS, RES_F64_OCC = 256, 2          # registers (VGPRs + AGPRs) per lane at most, waves per SIMD at least
RES_F32_REGS, RES_F32_OCC = 128, 4


def test_rff_grad_kernel_resources(tmp_path):
	"""The value / gradient kernels of rffgrad.hip (rff_grad_lds_kernel for d <= 64: 1 - 4 blocks of 16 output coordinates; rff_grad_kernel
	above): accumulators, x fragments, the prefetched W slab and the four sin / cos bodies of a 16-feature tile stay in registers --
	no scratch and no spill in any instantiation.  fp64 reaches 137 - 237 registers (VGPRs + AGPRs; the inlined libm sincos is the
	peak), fp32 (hardware trig) 66 - 125.  What the kernels rely on is the occupancy step those land on: two waves per SIMD in
	fp64 (<= 256 registers), four in fp32 (<= 128), and an LDS slab small enough never to be the limit (<= 18 KiB)."""
	out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-c", os.path.join(CSRC, "rffgrad.hip"),
						  "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
	blocks = {b.split()[0]: b for b in re.split(r"remark: Function Name: ", out)[1:]}
	get = lambda b, key: int(re.search(key + r": (\d+)", b).group(1))
	main = {n: b for n, b in blocks.items() if "rff_grad_lds_kernel" in n or "rff_grad_kernel" in n}
	assert len(main) == 10                   # fp64 / fp32 x (1, 2, 3, 4 coordinate blocks through LDS + the d > 64 form)
	for n, b in main.items():
		f64 = "kernelId" in n
		assert get(b, r"ScratchSize \[bytes/lane\]") == 0 and get(b, r"VGPRs Spill") == 0, n
		assert get(b, r"LDS Size \[bytes/block\]") <= 18 * 1024, n
		assert get(b, r"\bVGPRs") + get(b, r"\bAGPRs") <= (RES_F64_REGS if f64 else RES_F32_REGS), n
		assert get(b, r"Occupancy \[waves/SIMD\]") >= (RES_F64_OCC if f64 else RES_F32_OCC), n
	others = [b for n, b in blocks.items() if "rff_hess_kernel" in n or "rff_grad_finish_kernel" in n]
	assert len(others) == 4
	for b in others:
		assert get(b, r"ScratchSize \[bytes/lane\]") == 0 and get(b, r"LDS Size \[bytes/block\]") <= 2048


# ---------------------------------------------------------------- GPU: the C ABI

def _torch_ref(x, W, bias, fs, scale, C, hess=False):
	"""fp64 torch evaluation of the same sums on the device."""
	x, W, C = x.double(), W.double(), C.double()
	m = W.shape[0]
	q = x @ W.T
	a = scale * (fs.double() if fs is not None else torch.ones(m, dtype=torch.float64, device=x.device))
	if bias is not None:
		phi, dphi = a * torch.cos(q + bias.double()), -a * torch.sin(q + bias.double())
	else:
		h = m // 2
		phi = a * torch.cat([torch.cos(q[:, :h]), torch.sin(q[:, h:])], dim=1)
		dphi = a * torch.cat([-torch.sin(q[:, :h]), torch.cos(q[:, h:])], dim=1)
	C = C.expand(x.shape[0], m) if C.dim() == 1 else C
	H = -torch.einsum("tj,jk,jl->tkl", C * phi, W, W) if hess else None
	return (C * phi).sum(1), (C * dphi) @ W, H


def _dev(x, W, bias, fs, scale, C, order=1, combine=0, val=None, G=None, H=None, ldg=None):
	"""Raw call: x, W, C, G may be column windows of wider buffers (their strides are the leading dimensions)."""
	L = _lib()
	lib = L.load()
	n, d = x.shape
	m = W.shape[0]
	dt = L.dtype_code(x.dtype)
	work = torch.empty((int(lib.stpy_rff_grad_workspace_bytes(dt, n, d, m, order)),), dtype=torch.uint8, device=x.device)
	L.check(lib.stpy_rff_grad(dt, L.ptr(x), n, x.stride(0), d, L.ptr(W), W.stride(0), m, L.ptr(bias), L.ptr(fs), scale, L.ptr(C),
							  0 if C.dim() == 1 else C.stride(0), order, combine, L.ptr(val), L.ptr(G), G.stride(0) if ldg is None else ldg, L.ptr(H),
							  L.ptr(work), work.numel(), L.stream_ptr()), "stpy_rff_grad")


def _problem(n, m, d, dev, seed, dtype=torch.float64):
	"""x ~ U(-1, 1), W ~ N(0, 1) / gamma with gamma = 0.5 sqrt(d), C ~ N(0, 1); every matrix inside a wider buffer."""
	gen = torch.Generator(device="cpu").manual_seed(seed)
	r = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
	p = dict(
		xb=(torch.rand((n, d + 3), generator=gen, dtype=torch.float64) * 2 - 1), Wb=r(m, d + 5) / (0.5 * np.sqrt(d)), Cb=r(n, m + 7), row=r(m),
		bias=torch.rand((m,), generator=gen, dtype=torch.float64) * 2 * np.pi, fs=0.5 + torch.rand((m,), generator=gen, dtype=torch.float64),
		G0=r(n, d + 2), v0=r(n))
	p = {k: v.to(device=dev, dtype=dtype) for k, v in p.items()}
	p["x"], p["W"], p["C"] = p["xb"][:, :d], p["Wb"][:, :d], p["Cb"][:, :m]
	p["Cc"] = p["C"].contiguous()
	return p


# (bias, feat_scale, coefficients, val requested, ADD); coefficients: 0 = rows inside a wider matrix (ldc = m + 7), 1 = ONE shared row
# (ldc = 0), 2 = a contiguous n x m matrix (ldc = m: rows aligned for vector loads when m % 4 == 0)
VARIANTS = [(False, False, 0, True, False), (True, True, 0, False, True), (False, True, 1, True, False), (True, False, 1, True, True),
			(False, True, 2, True, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 127, 1000])
@pytest.mark.parametrize("m", [2, 64, 999, 1000, 4098])
@pytest.mark.parametrize("d", [1, 3, 16, 40, 64, 100])          # (100: the d > 64 kernel, two blocks of output coordinates)
def test_gpu_rff_grad_ragged(gpu_device, n, m, d):
	p = _problem(n, m, d, gpu_device, n * 1000003 + m * 101 + d)
	scale = 0.7
	for use_bias, use_fs, shared, want_val, add in VARIANTS:
		use_bias = use_bias or m % 2 == 1                        # an odd m only with a bias
		bias, fs = (p["bias"] if use_bias else None), (p["fs"] if use_fs else None)
		C = (p["C"], p["row"], p["Cc"])[shared]
		outs = []
		for _ in range(2):
			Gb = p["G0"].clone() if add else torch.full_like(p["G0"], float("nan"))
			val = (p["v0"].clone() if add else torch.full_like(p["v0"], float("nan"))) if want_val else None
			_dev(p["x"], p["W"], bias, fs, scale, C, combine=1 if add else 0, val=val, G=Gb[:, :d])
			outs.append((Gb, val))
		assert torch.equal(outs[0][0][:, :d], outs[1][0][:, :d]), "two calls differ"
		Gb, val = outs[0]
		assert torch.equal(Gb[:, d:], p["G0"][:, d:]) or (not add and bool(torch.isnan(Gb[:, d:]).all())), "columns past d written"
		rv, rG, _ = _torch_ref(p["x"], p["W"], bias, fs, scale, C)
		if add:
			rv, rG = rv + p["v0"], rG + p["G0"][:, :d]
		e = rel_err(Gb[:, :d].cpu().numpy(), rG.cpu().numpy())
		print("rff_grad n=%d m=%d d=%d %s: G %.2e" % (n, m, d, (use_bias, use_fs, shared, want_val, add), e))
		assert e < 1e-11, (n, m, d, use_bias, use_fs, shared, add)
		if want_val:
			assert torch.equal(outs[0][1], outs[1][1])
			assert rel_err(val.cpu().numpy(), rv.cpu().numpy()) < 1e-11, (n, m, d, use_bias, use_fs, shared, add)
	if n == 1000 and m in (64, 1000, 4098):                   # fp32 against fp64 on the same inputs
		q = _problem(n, m, d, gpu_device, n * 1000003 + m * 101 + d, dtype=torch.float32)
		for shared in (False, True):
			C32 = q["row"] if shared else q["C"]
			G32 = torch.full_like(q["G0"], float("nan"))
			v32 = torch.full_like(q["v0"], float("nan"))
			_dev(q["x"], q["W"], None, q["fs"], scale, C32, val=v32, G=G32[:, :d])
			rv, rG, _ = _torch_ref(q["x"], q["W"], None, q["fs"], scale, C32)
			eg, ev = rel_err(G32[:, :d].double().cpu().numpy(), rG.cpu().numpy()), rel_err(v32.double().cpu().numpy(), rv.cpu().numpy())
			print("rff_grad fp32 n=%d m=%d d=%d shared=%s: G %.2e val %.2e" % (n, m, d, shared, eg, ev))
			assert eg < 1e-3 and ev < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("m", [2, 64, 1000, 4098])
@pytest.mark.parametrize("d", [1, 3, 16, 40, 64])
def test_gpu_rff_grad_hessian(gpu_device, n, m, d):
	p = _problem(n, m, d, gpu_device, 77 + n * 1000003 + m * 101 + d)
	ldg = d + 2
	gen = torch.Generator(device="cpu").manual_seed(d)
	H0 = torch.randn((n, ldg, ldg), generator=gen, dtype=torch.float64).to(gpu_device)
	for (use_bias, use_fs, shared, _, add) in VARIANTS:
		bias, fs = (p["bias"] if use_bias else None), (p["fs"] if use_fs else None)
		C = (p["C"], p["row"], p["Cc"])[shared]
		outs = []
		for _ in range(2):
			Gb = p["G0"].clone() if add else torch.full_like(p["G0"], float("nan"))
			Hb = H0.clone() if add else torch.full_like(H0, float("nan"))
			val = p["v0"].clone() if add else torch.full_like(p["v0"], float("nan"))
			_dev(p["x"], p["W"], bias, fs, 1.3, C, order=2, combine=1 if add else 0, val=val, G=Gb[:, :d], H=Hb)
			outs.append((Gb, Hb, val))
		assert all(torch.equal(a, b) or bool(torch.isnan(a).any()) for a, b in zip(outs[0], outs[1]))
		assert torch.equal(outs[0][1][:, :d, :d], outs[1][1][:, :d, :d])
		Gb, Hb, val = outs[0]
		rv, rG, rH = _torch_ref(p["x"], p["W"], bias, fs, 1.3, C, hess=True)
		if add:
			rv, rG, rH = rv + p["v0"], rG + p["G0"][:, :d], rH + H0[:, :d, :d]
		assert rel_err(val.cpu().numpy(), rv.cpu().numpy()) < 1e-11
		assert rel_err(Gb[:, :d].cpu().numpy(), rG.cpu().numpy()) < 1e-11
		assert rel_err(Hb[:, :d, :d].cpu().numpy(), rH.cpu().numpy()) < 1e-11, (n, m, d, use_bias, use_fs, shared, add)


@pytest.mark.gpu
@pytest.mark.parametrize("m,d", [(64, 3), (1000, 16), (999, 5), (4098, 64)])
def test_gpu_rff_grad_value_matches_embed(gpu_device, m, d):
	"""val is stpy_rff_embed of the same operands contracted with C."""
	L = _lib()
	p = _problem(300, m, d, gpu_device, m + d)
	for bias, fs in ((None, None), (p["bias"], p["fs"])) if m % 2 == 0 else ((p["bias"], None),):
		Phi = L.rff_embed(p["x"], p["W"], m, 0.9, bias=bias, feat_scale=fs)
		val = torch.empty((300,), dtype=torch.float64, device=gpu_device)
		G = torch.empty((300, d), dtype=torch.float64, device=gpu_device)
		L.rff_grad(p["x"], p["W"], m, 0.9, p["C"], G, bias=bias, feat_scale=fs, val=val)
		assert rel_err(val.cpu().numpy(), (Phi * p["C"]).sum(1).cpu().numpy()) < 1e-12


# ---------------------------------------------------------------- GPU: embeddings and the estimator against G18

@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_gpu_estimator_against_reference(gpu_device, case):
	g = golden("G18_kf_input_grad")
	KF = make_model(case, g)
	xb = g[case + "_xb"]
	for cuda in (False, True):
		xt = torch.from_numpy(xb).to(gpu_device if cuda else "cpu").requires_grad_(True)
		mu, std = KF.mean_std(xt)
		assert mu.is_cuda == cuda and tuple(mu.shape) == (6, 1) and mu.grad_fn is not None
		assert rel_err(mu.detach().cpu().numpy(), g[case + "_mu"]) < 1e-8
		mu.sum().backward()
		assert xt.grad.is_cuda == cuda and rel_err(xt.grad.cpu().numpy(), g[case + "_dmu_sum"]) < 1e-8
		xt.grad = None
		mu, std = KF.mean_var(xt)
		assert rel_err(std.detach().cpu().numpy(), g[case + "_std"]) < 1e-8
		std.sum().backward()
		assert rel_err(xt.grad.cpu().numpy(), g[case + "_dstd_sum"]) < 1e-8
		xt.grad = None
		mu, std = KF.mean_std(xt)
		(mu.sum() + std.sum()).backward()
		assert rel_err(xt.grad.cpu().numpy(), g[case + "_dmu_sum"] + g[case + "_dstd_sum"]) < 1e-8
		xt.grad = None
		KF.mean(xt).sum().backward()
		assert rel_err(xt.grad.cpu().numpy(), g[case + "_dmu_sum"]) < 1e-8
		xt.grad = None
		KF.ucb(xt).sum().backward()                                 # beta = 2 (beta_fun None)
		assert rel_err(xt.grad.cpu().numpy(), g[case + "_dmu_sum"] + np.sqrt(2.0) * g[case + "_dstd_sum"]) < 1e-8
		xt.grad = None
		KF.lcb(xt).sum().backward()
		assert rel_err(xt.grad.cpu().numpy(), g[case + "_dmu_sum"] - np.sqrt(2.0) * g[case + "_dstd_sum"]) < 1e-8
	# the private Hessian helper against the reference's mean_gradient_hessian(hessian=True)
	G, H = KF._mean_hessian(torch.from_numpy(g[case + "_pts"]))
	assert tuple(H.shape) == (4,) + (xb.shape[1],) * 2 and not H.is_cuda
	assert rel_err(G.numpy(), g[case + "_grad"]) < 1e-8 and rel_err(H.numpy(), g[case + "_hess"]) < 1e-8
	# without requires_grad nothing changes: same numbers bit for bit, no graph
	mu0, std0 = KF.mean_std(torch.from_numpy(xb))
	mu1, std1 = KF.mean_std(torch.from_numpy(xb).requires_grad_(True))
	assert mu0.grad_fn is None and std0.grad_fn is None
	assert torch.equal(mu0, mu1.detach()) and torch.equal(std0, std1.detach())
	with torch.no_grad():
		assert KF.mean_std(torch.from_numpy(xb).requires_grad_(True))[0].grad_fn is None
	# theta and Z of the gradient's closed form
	theta, Z = KF.theta_mean(var=True)
	assert rel_err(theta.numpy(), g[case + "_theta"]) < 1e-8 and rel_err(Z.numpy(), g[case + "_Z"]) < 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("primal", [True, False])
def test_gpu_sigma_gradient_after_refit(gpu_device, primal):
	"""The sigma-gradient reads V^-1 (primal) / K^-1 (dual), built once per factor by the first gradient after a fit.  Model A takes a
	gradient (which fills that inverse), then gets 3 queued points and takes the gradient again; model B gets the same fit and the
	same points and only then its first gradient.  Both final factors come from the same launches on the same data and the library's
	reductions are fixed-order, so the two gradients are equal bit for bit; an inverse that outlived A's first factor would differ
	in the first digit.  m = 64 features, 40 + 3 points: primal=False stays in the dual form (43 < 64)."""
	import stpy_amd
	from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures
	rng = np.random.RandomState(21)
	x = rng.uniform(-1, 1, size=(43, 2))
	y = np.sin(3 * x[:, :1]) * np.cos(2 * x[:, 1:]) + 0.05 * rng.normal(size=(43, 1))
	x, y, xt = torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(rng.uniform(-1, 1, size=(5, 2)))
	np.random.seed(8)
	emb = stpy_amd.RFFEmbedding(gamma=0.5, m=64, d=2)

	def model():
		KF = KernelizedFeatures(embedding=emb, m=emb.get_m(), s=0.1, lam=1.0, d=2, primal=primal)
		KF.fit_gp(x[:40], y[:40])
		return KF

	def sigma_grad(KF):
		z = xt.clone().requires_grad_(True)
		KF.mean_std(z)[1].sum().backward()
		return z.grad

	A, B = model(), model()
	before = sigma_grad(A)
	for KF in (A, B):
		KF.add_data_point(x[40:], y[40:])
		assert KF.fitted is False                                 # queued: folded in by the next prediction
	gA, gB = sigma_grad(A), sigma_grad(B)
	assert A.n == B.n == 43 and A.dual == B.dual == (not primal)
	assert bool(torch.isfinite(gA).all()) and not torch.equal(gA, before)
	assert torch.equal(gA, gB), float((gA - gB).abs().max() / gB.abs().max())


@pytest.mark.gpu
def test_gpu_quadrature_derivatives(gpu_device):
	import stpy_amd
	g = golden("G18_kf_input_grad")
	emb = make_embedding("hermite", g)
	xb = torch.from_numpy(g["hermite_xb"])
	z1, z2 = emb.derivative_1(xb), emb.derivative_2(xb)
	assert tuple(z1.shape) == (2, 72, 6) and tuple(z2.shape) == (2, 2, 72, 6) and not z1.is_cuda
	assert rel_err(z1.numpy(), g["hermite_d1"]) < 1e-8 and rel_err(z2.numpy(), g["hermite_d2"]) < 1e-8
	assert emb.derivative_1(xb.to(gpu_device)).is_cuda
	cosine = stpy_amd.QuadratureEmbedding(gamma=0.5, m=6, d=1, cosine=True)
	for f in (cosine.derivative_1, cosine.derivative_2):
		with pytest.raises(NotImplementedError):
			f(torch.zeros((2, 1), dtype=torch.float64))
	# the contraction of the Jacobian with coefficients is value_grad
	C = torch.from_numpy(np.random.RandomState(1).normal(size=(6, 72)))
	val, G, H = emb.value_grad(xb, C, hessian=True)
	assert val.is_cuda and rel_err(G.cpu().numpy(), np.einsum("kjt,tj->tk", g["hermite_d1"], C.numpy())) < 1e-8
	assert rel_err(H.cpu().numpy(), np.einsum("kljt,tj->tkl", g["hermite_d2"], C.numpy())) < 1e-8


@pytest.mark.gpu
def test_gpu_concat_and_biased_embeddings(gpu_device):
	import stpy_amd.embeddings.embedding as stpy_amd
	rng = np.random.RandomState(4)
	np.random.seed(9)
	e1 = stpy_amd.RFFEmbedding(gamma=0.6, m=32, d=3, kappa=1.1)
	e2 = stpy_amd.RFFEmbedding(gamma=1.4, m=64, d=3, kappa=0.7)
	eb = stpy_amd.RFFEmbedding(gamma=0.9, m=48, d=3, kappa=1.3, biased=True)
	x = rng.uniform(-1, 1, size=(50, 3))
	xt = torch.from_numpy(x)
	cat = stpy_amd.ConcatEmbedding([e1, e2])
	for C in (rng.normal(size=(50, 96)), rng.normal(size=(96,))):
		val, G, H = cat.value_grad(xt, torch.from_numpy(C), hessian=True)
		parts = [value_grad_hess(np_operands(e), x, C[..., sl]) for e, sl in ((e1, slice(0, 32)), (e2, slice(32, 96)))]
		for got, k in ((val, 0), (G, 1), (H, 2)):
			assert rel_err(got.cpu().numpy(), parts[0][k] + parts[1][k]) < 1e-10
		assert rel_err(val.cpu().numpy(), (cat.embed(xt).numpy() * C).sum(1)) < 1e-10
	Cb = rng.normal(size=(50, 48))
	val, G, H = eb.value_grad(xt, torch.from_numpy(Cb), hessian=True)
	for got, want in zip((val, G, H), value_grad_hess(np_operands(eb), x, Cb)):
		assert rel_err(got.cpu().numpy(), want) < 1e-10
	assert rel_err(val.cpu().numpy(), (eb.embed(xt).numpy().T * Cb).sum(1)) < 1e-10          # (biased embed returns (m, n))


# ---------------------------------------------------------------- GPU: sample_and_optimize

def _sample_problem(d):
	import stpy_amd
	from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures
	rng = np.random.RandomState(7 + d)                         # the data of test_posterior_grad._ucb_problem
	x = rng.uniform(-1, 1, size=(25, d))
	y = np.sin(3 * x[:, :1]) * np.cos(2 * x[:, -1:]) + 0.05 * rng.normal(size=(25, 1))
	if d == 1:
		np.random.seed(5)
		emb = stpy_amd.RFFEmbedding(gamma=0.4, m=64, d=1)
	else:
		emb = stpy_amd.HermiteEmbedding(gamma=0.4, m=2 * 12 ** 2, d=2)
	KF = KernelizedFeatures(embedding=emb, m=emb.get_m(), s=0.05, lam=1.0, d=d, bounds=[(-1.0, 1.0)] * d)
	KF.fit_gp(torch.from_numpy(x), torch.from_numpy(y))
	return KF, emb


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [11, 12, 13])
@pytest.mark.parametrize("d", [1, 2])
def test_gpu_sample_and_optimize(gpu_device, d, seed):
	KF, emb = _sample_problem(d)
	torch.manual_seed(seed)
	theta = KF.sample_theta().numpy().reshape(-1)
	torch.manual_seed(seed)
	np.random.seed(3)
	sol, val = KF.sample_and_optimize()
	s = sol.numpy()
	assert s.shape == (d,) and sol.dtype == torch.float64 and tuple(val.shape) == (1,)
	assert np.all(s >= -1.0) and np.all(s <= 1.0)
	phi = emb.embed(torch.from_numpy(s.reshape(1, d))).numpy()
	assert abs(float(val[0]) - float((phi @ theta)[0])) < 1e-10
	grid = np.stack(np.meshgrid(*[np.linspace(-1, 1, 401 if d == 1 else 201)] * d, indexing="ij"), -1).reshape(-1, d)
	gmax = float((emb.embed(torch.from_numpy(grid)).numpy() @ theta).max())
	_, g, _ = value_grad_hess(np_operands(emb), s.reshape(1, d), theta)
	proj = np.clip(s + g[0], -1.0, 1.0) - s                    # projected gradient of the maximisation
	print("sample_and_optimize d=%d seed=%d: value - grid max %.3e, projected gradient %.3e, %d evaluations"
		  % (d, seed, float(val[0]) - gmax, np.abs(proj).max(), KF._last_optimize_evaluations))
	assert float(val[0]) >= gmax - 1e-6
	assert np.abs(proj).max() <= 1e-5
	with pytest.raises(AssertionError, match="Wrong optimizer"):
		KF.sample_and_optimize(minimizer="BFGS")


@pytest.mark.gpu
def test_gpu_refused_names_point_to_what_works(gpu_device):
	g = golden("G18_kf_input_grad")
	KF = make_model("rff", g)
	xb = torch.from_numpy(g["rff_xb"])
	for call in (lambda: KF.mean_std_grad(xb), lambda: KF.mean_gradient_hessian(xb[:1]), lambda: KF.gradient_mean_var(xb[:1]), lambda: KF.ucb_optimize(2.0)):
		with pytest.raises(NotImplementedError, match="KernelizedFeatures") as ei:
			call()
		assert "sample_and_optimize" in str(ei.value) and "requires_grad" in str(ei.value)
