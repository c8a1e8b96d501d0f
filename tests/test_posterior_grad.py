"""
Input gradients of the GP posterior: stpy_gram_grad / stpy_trsm_right_ln (csrc/grad.hip) and the GaussianProcess surface built
on them (mean_std / mean / ucb autograd, mean_std_grad, mean_gradient_hessian, gradient_mean_var, ucb_optimize).

The closed forms below (psi, chi, the product rule, the chain rule through a full covariance map) are the checker: on the CPU
they must reproduce the reference's autograd numbers in G17 (tests/golden/make_golden_grad.py); on the GPU the device results
must reproduce them, and the kinds the reference cannot differentiate (Matern) are checked against the closed forms alone.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import golden, rel_err

# ---------------------------------------------------------------- the G17 kernels (same table as tests/golden/make_golden_grad.py)
D = 3
COV = [[0.9, 0.2, 0.0], [-0.1, 1.3, 0.3], [0.2, 0.0, 0.7]]
CASES = {
	"se": [("-", dict(kernel_name="squared_exponential", gamma=0.7, kappa=1.3))],
	"ard": [("-", dict(kernel_name="ard", ard_gamma=[0.5, 0.9, 1.4], kappa=1.1))],
	"ard_groups": [("-", dict(kernel_name="ard", ard_gamma=[0.6, 0.8, 1.2], kappa=1.1, groups=[[0, 1], [2]]))],
	"se_plus_linear": [("-", dict(kernel_name="squared_exponential", gamma=0.8, kappa=1.0)),
					   ("+", dict(kernel_name="linear", kappa=0.5))],
	"se_times_se": [("-", dict(kernel_name="squared_exponential", gamma=0.8, kappa=1.0)),
					("*", dict(kernel_name="squared_exponential", gamma=2.0, kappa=0.7, group=[1, 2]))],
	"poly": [("-", dict(kernel_name="polynomial", power=3, kappa=0.4))],
	"fullcov_se": [("-", dict(kernel_name="full_covariance_se", cov=COV, kappa=1.2))],
}


def make_kernel(spec, d=D):
	from stpy_amd import KernelFunction
	k = None
	for op, kw in spec:
		kw = dict(kw, d=d)
		if "ard_gamma" in kw:
			kw["ard_gamma"] = torch.tensor(kw["ard_gamma"], dtype=torch.float64)
		if "cov" in kw:
			kw["cov"] = torch.tensor(kw["cov"], dtype=torch.float64)
		item = KernelFunction(**kw)
		k = item if k is None else (k + item if op == "+" else k * item)
	return k


# ---------------------------------------------------------------- closed forms (NumPy, fp64)
SQ3, SQ5 = np.sqrt(3.0), np.sqrt(5.0)


def radial(kind, r2):
	"""phi, psi = phi'(r)/r, chi = psi'(r)/r per family (kappa = 1)."""
	r = np.sqrt(r2)
	if kind == 0:
		e = np.exp(-0.5 * r2)
		return e, -e, e
	if kind == 1:
		e = np.exp(-r)
		with np.errstate(divide="ignore", invalid="ignore"):
			psi = np.where(r > 0, -e / np.where(r > 0, r, 1.0), 0.0)
		return e, psi, np.full_like(r, np.nan)
	if kind == 2:
		e = np.exp(-SQ3 * r)
		return (1 + SQ3 * r) * e, -3.0 * e, np.full_like(r, np.nan)
	e = np.exp(-SQ5 * r)
	return (1 + SQ5 * r + 5.0 * r2 / 3.0) * e, -(5.0 / 3.0) * (1 + SQ5 * r) * e, (25.0 / 3.0) * e


def term_kgh(term, A, X):
	"""value (m, n), gradient in A (m, n, D) and Hessian in A (m, n, D, D) of one resolved kernel term."""
	m, n, Dall = A.shape[0], X.shape[0], A.shape[1]
	g = list(term['group'])
	kind, degree = term['kind'] & 0xff, term['kind'] >> 8
	kap = term['kappa']
	G = np.zeros((m, n, Dall))
	H = np.zeros((m, n, Dall, Dall))
	if term['premap'] is not None:
		cov = term['premap'].numpy()
		za, zx = A[:, g] @ cov, X[:, g] @ cov
		U = za[:, None, :] - zx[None, :, :]
		phi, psi, chi = radial(kind, (U * U).sum(-1))
		Gz = kap * psi[..., None] * U
		Hz = kap * (psi[..., None, None] * np.eye(cov.shape[1]) + chi[..., None, None] * U[..., :, None] * U[..., None, :])
		G[:, :, g] = Gz @ cov.T
		Hg = np.einsum("ap,mnpq,bq->mnab", cov, Hz, cov)
		for a_i, a in enumerate(g):
			for b_i, b in enumerate(g):
				H[:, :, a, b] = Hg[:, :, a_i, b_i]
		return kap * phi, G, H
	il = np.asarray(term['inv_ls'])
	As, Xs = A[:, g] * il, X[:, g] * il
	if kind in (4, 5):
		s = As @ Xs.T
		Xl = Xs * il                                            # d s / d A_g
		if kind == 4:
			k = kap * s + term['offset']
			f1, f2 = np.full_like(s, kap), np.zeros_like(s)
		else:
			b = s + term['offset']
			k = kap * b ** degree
			f1 = kap * degree * b ** (degree - 1)
			f2 = kap * degree * (degree - 1) * b ** (degree - 2) if degree >= 2 else np.zeros_like(s)
		G[:, :, g] = f1[..., None] * Xl[None, :, :]
		Hg = f2[..., None, None] * Xl[None, :, :, None] * Xl[None, :, None, :]
	else:
		U = As[:, None, :] - Xs[None, :, :]
		phi, psi, chi = radial(kind, (U * U).sum(-1))
		k = kap * phi
		G[:, :, g] = kap * psi[..., None] * U * il
		Hg = kap * (psi[..., None, None] * np.eye(len(g)) + chi[..., None, None] * U[..., :, None] * U[..., None, :]) * np.outer(il, il)
	for a_i, a in enumerate(g):
		for b_i, b in enumerate(g):
			H[:, :, a, b] = Hg[:, :, a_i, b_i]
	return k, G, H


def kernel_kgh(kernel, A, X):
	"""The + / * chain of the kernel's items (kernels.py:146-157) with the sum and product rules."""
	K = G = H = None
	for it in kernel._resolve({}):
		k = sum(term_kgh(t, A, X)[0] for t in it['terms'])
		g = sum(term_kgh(t, A, X)[1] for t in it['terms'])
		h = sum(term_kgh(t, A, X)[2] for t in it['terms'])
		if K is None:
			K, G, H = k, g, h
		elif it['op'] == "+":
			K, G, H = K + k, G + g, H + h
		else:
			H = (H * k[..., None, None] + G[..., :, None] * g[..., None, :] + g[..., :, None] * G[..., None, :] + K[..., None, None] * h)
			G = G * k[..., None] + K[..., None] * g
			K = K * k
	return K, G, H


def posterior_grads(kernel, x, y, s, xt):
	"""mu, std, d mu (m, D), d std (m, D), Hessian of mu (m, D, D) of the exact GP posterior, closed forms."""
	Kxx = kernel_kgh(kernel, x, x)[0] + s * s * np.eye(x.shape[0])
	alpha = np.linalg.solve(Kxx, y).reshape(-1)
	Ks, Gs, Hs = kernel_kgh(kernel, xt, x)
	W = np.linalg.solve(Kxx, Ks.T).T                              # (m, n) = K* K^-1
	mu = Ks @ alpha
	kd = np.array([kernel_kgh(kernel, xt[i:i + 1], xt[i:i + 1])[0][0, 0] for i in range(xt.shape[0])])
	gself = np.stack([2.0 * kernel_kgh(kernel, xt[i:i + 1], xt[i:i + 1])[1][0, 0] for i in range(xt.shape[0])])
	var = kd - (W * Ks).sum(1)
	std = np.sqrt(var)
	dmu = np.einsum("i,mid->md", alpha, Gs)
	dvar = gself - 2.0 * np.einsum("mi,mid->md", W, Gs)
	dstd = dvar / (2.0 * std[:, None])
	hmu = np.einsum("i,miab->mab", alpha, Hs)
	return mu, std, dmu, dstd, hmu


# ---------------------------------------------------------------- CPU: argument checks and the closed forms against the reference

def _lib():
	from stpy_amd import _lib as L
	return L


def _gg(lib, kind=0, dtype=0, n=5, m=4, d=3, order=1, G=16, H=None, work=16, work_bytes=1 << 20):
	p = ctypes.c_void_p(16)
	return lib.stpy_gram_grad(kind, dtype, p, n, 8, p, m, 8, d, None, p, 1.0, 0.0, p, None, None, 0, None, order, 0,
							  ctypes.c_void_p(G) if G else None, 8, ctypes.c_void_p(H) if H else None, ctypes.c_void_p(work) if work else None,
							  work_bytes, None)


def test_gram_grad_argument_checks():
	L = _lib()
	lib = L.load()
	assert _gg(lib, kind=9) == -1
	assert b"kind" in lib.stpy_last_error_string()
	assert _gg(lib, kind=L.K_POLY) == -1                     # polynomial without a degree
	assert _gg(lib, dtype=7) == -2
	assert _gg(lib, d=0) == -9
	assert _gg(lib, d=-2) == -9
	assert _gg(lib, kind=L.K_MATERN12, order=2, H=16) == -19
	assert b"Hessian" in lib.stpy_last_error_string()
	assert _gg(lib, kind=L.K_MATERN32, order=2, H=16) == -19
	assert _gg(lib, order=3) == -19
	assert _gg(lib, G=0) == -21
	assert _gg(lib, order=2, H=0) == -23
	assert _gg(lib, work=0) == -24
	assert _gg(lib, work_bytes=8) == -25
	# empty problems return 0 without looking at a pointer
	assert lib.stpy_gram_grad(9, 7, None, 0, 0, None, 4, 0, 0, None, None, 1.0, 0.0, None, None, None, 0, None, 5, 9, None, 0, None, None, 0, None) == 0
	assert lib.stpy_gram_grad(9, 7, None, 5, 0, None, 0, 0, 0, None, None, 1.0, 0.0, None, None, None, 0, None, 5, 9, None, 0, None, None, 0, None) == 0
	assert lib.stpy_gram_grad_workspace_bytes(0, 0, 10, 3, 1) == 0
	assert lib.stpy_gram_grad_workspace_bytes(0, 4096, 65536, 16, 1) > 0
	assert lib.stpy_gram_grad_workspace_bytes(1, 4096, 65536, 16, 1) * 2 == lib.stpy_gram_grad_workspace_bytes(0, 4096, 65536, 16, 1)


def test_trsm_right_ln_argument_checks():
	lib = _lib().load()
	p = ctypes.c_void_p(16)
	assert lib.stpy_trsm_right_ln(0, 0, 128, None, 128, None, 0, None, 128, 0, 0, None, 0, None) == 0
	assert lib.stpy_trsm_right_ln(0, 4, 100, p, 100, p, 1 << 20, p, 100, 0, 0, None, 0, None) == -3        # not tile-aligned
	assert lib.stpy_trsm_right_ln(0, 4, 128, p, 128, p, 10, p, 128, 0, 0, None, 0, None) == -7             # winv too small
	assert lib.stpy_trsm_right_ln(0, 4, 128, None, 128, p, 1 << 20, p, 128, 0, 0, None, 0, None) == -4
	assert lib.stpy_trsm_ln_factor(0, 0, None, 0, None, 0, None, 0, None, None) == 0
	assert lib.stpy_trsm_ln_factor(0, 200, p, 200, p, 1 << 20, p, 200, p, None) == -2
	assert lib.stpy_trsm_ln_factor(0, 256, p, 200, p, 1 << 20, p, 256, p, None) == -4


@pytest.mark.parametrize("case", sorted(CASES))
def test_closed_forms_reproduce_reference(case):
	g = golden("G17_posterior_grad")
	k = make_kernel(CASES[case])
	x, y, s = g["x"], g["y"], float(g["s"])
	for j, p in enumerate(g["pts"]):
		_, _, dmu, _, hmu = posterior_grads(k, x, y, s, p.reshape(1, -1))
		assert np.abs(dmu[0] - g[case + "_grad"][j]).max() < 1e-10 * max(1.0, np.abs(g[case + "_grad"][j]).max())
		assert np.abs(hmu[0] - g[case + "_hess"][j]).max() < 1e-10 * max(1.0, np.abs(g[case + "_hess"][j]).max())
	mu, std, dmu, dstd, _ = posterior_grads(k, x, y, s, g["xb"])
	assert rel_err(mu, g[case + "_mu"].reshape(-1)) < 1e-10
	assert rel_err(std, g[case + "_std"].reshape(-1)) < 1e-10
	assert rel_err(dmu, g[case + "_dmu_sum"]) < 1e-10
	assert rel_err(dstd, g[case + "_dstd_sum"]) < 1e-10


# ---------------------------------------------------------------- GPU
def _gp(kernel, x, y, s=0.1, dtype=torch.float64):
	from stpy_amd import GaussianProcess
	GP = GaussianProcess(kernel=kernel, s=s, d=x.shape[1])
	GP.fit_gp(torch.from_numpy(x).to(dtype), torch.from_numpy(y).to(dtype))
	return GP


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_gpu_against_reference(gpu_device, case):
	g = golden("G17_posterior_grad")
	GP = _gp(make_kernel(CASES[case]), g["x"], g["y"], float(g["s"]))
	for j, p in enumerate(g["pts"]):
		pt = torch.from_numpy(p.reshape(1, -1))
		if case == "se_times_se":
			with pytest.raises(NotImplementedError):
				GP.mean_gradient_hessian(pt, hessian=True)
			gr = GP.mean_gradient_hessian(pt)
		else:
			gr, h = GP.mean_gradient_hessian(pt, hessian=True)
			assert tuple(h.shape) == (D, D)
			assert rel_err(h.numpy(), g[case + "_hess"][j]) < 1e-8
		assert tuple(gr.shape) == (D,) and not gr.is_cuda
		assert rel_err(gr.numpy(), g[case + "_grad"][j]) < 1e-8
		assert rel_err(GP.gradient_mean_var(pt).numpy(), g[case + "_grad"][j]) < 1e-8
	for cuda in (False, True):
		xt = torch.from_numpy(g["xb"]).to(gpu_device if cuda else "cpu").requires_grad_(True)
		mu, std = GP.mean_std(xt)
		assert mu.is_cuda == cuda and tuple(mu.shape) == (6, 1)
		mu.sum().backward()
		assert rel_err(xt.grad.cpu().numpy(), g[case + "_dmu_sum"]) < 1e-8
		xt.grad = None
		mu, std = GP.mean_var(xt)
		assert rel_err(std.detach().cpu().numpy(), g[case + "_std"]) < 1e-8
		std.sum().backward()
		assert rel_err(xt.grad.cpu().numpy(), g[case + "_dstd_sum"]) < 1e-8
	xt = torch.from_numpy(g["xb"]).requires_grad_(True)
	GP.ucb(xt).sum().backward()
	assert rel_err(xt.grad.numpy(), g[case + "_dmu_sum"] + 2.0 * g[case + "_dstd_sum"]) < 1e-8
	xt.grad = None
	GP.mean(xt).sum().backward()
	assert rel_err(xt.grad.numpy(), g[case + "_dmu_sum"]) < 1e-8
	dmu, dstd = GP.mean_std_grad(torch.from_numpy(g["xb"]))
	assert rel_err(dmu.numpy(), g[case + "_dmu_sum"]) < 1e-8 and rel_err(dstd.numpy(), g[case + "_dstd_sum"]) < 1e-8
	# without requires_grad nothing changes: same numbers, no graph
	mu0, std0 = GP.mean_std(torch.from_numpy(g["xb"]))
	assert mu0.grad_fn is None and torch.equal(mu0, mu.detach().cpu()) and torch.equal(std0, std.detach().cpu())


MATERN = {
	"matern05": [("-", dict(kernel_name="matern", gamma=0.6, nu=0.5, kappa=1.2))],
	"matern15": [("-", dict(kernel_name="matern", gamma=0.7, nu=1.5, kappa=0.9))],
	"matern25": [("-", dict(kernel_name="matern", gamma=0.8, nu=2.5, kappa=1.1))],
	"ard_matern25": [("-", dict(kernel_name="ard_matern", ard_gamma=[0.5, 0.9, 1.3], nu=2.5, kappa=1.0))],
	"ard_matern15": [("-", dict(kernel_name="ard_matern", ard_gamma=[0.7, 1.1, 0.6], nu=1.5, kappa=1.0))],
	"fullcov_matern25": [("-", dict(kernel_name="full_covariance_matern", cov=COV, nu=2.5, kappa=1.2))],
	"fullcov_matern15": [("-", dict(kernel_name="full_covariance_matern", cov=COV, nu=1.5, kappa=1.2))],
	"se_plus_matern05": [("-", dict(kernel_name="squared_exponential", gamma=0.8, kappa=1.0)),
						 ("+", dict(kernel_name="matern", gamma=0.6, nu=0.5, kappa=0.5))],
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(MATERN))
def test_gpu_matern_closed_forms(gpu_device, case):
	g = golden("G17_posterior_grad")
	k = make_kernel(MATERN[case])
	x, y, s = g["x"], g["y"], float(g["s"])
	GP = _gp(k, x, y, s)
	xb = g["xb"]                                   # continuous uniform draws: no test point coincides with a training point
	_, std, dmu, dstd, hmu = posterior_grads(k, x, y, s, xb)
	xt = torch.from_numpy(xb).requires_grad_(True)
	m_, s_ = GP.mean_std(xt)
	(m_.sum() + 0.0 * s_.sum()).backward()
	assert rel_err(xt.grad.numpy(), dmu) < 1e-8
	dm, ds = GP.mean_std_grad(torch.from_numpy(xb))
	assert rel_err(dm.numpy(), dmu) < 1e-8 and rel_err(ds.numpy(), dstd) < 1e-8
	if "05" in case or "15" in case:
		with pytest.raises(NotImplementedError, match="Matern"):
			GP.mean_gradient_hessian(torch.from_numpy(xb[:1]), hessian=True)
	else:
		_, h = GP.mean_gradient_hessian(torch.from_numpy(xb[:1]), hessian=True)
		assert rel_err(h.numpy(), hmu[0]) < 1e-8


def _torch_grad(kind, x, xt, il, kappa, offset, alpha, u, Wt, v, hess=False):
	"""fp64 torch evaluation of the same sums on the GPU, row chunks (SE / Matern 5/2 / polynomial)."""
	out, outh = [], []
	for r0 in range(0, xt.shape[0], 64):
		a = xt[r0:r0 + 64] * il
		c = torch.zeros((a.shape[0], x.shape[0]), dtype=torch.float64, device=x.device)
		if alpha is not None:
			c += u[r0:r0 + 64, None] * alpha[None, :]
		if Wt is not None:
			c += v[r0:r0 + 64, None] * Wt[r0:r0 + 64, :x.shape[0]]
		xs = x * il
		if kind & 0xff == 5:
			p = kind >> 8
			b = a @ xs.T + offset
			w1, w2 = c * kappa * p * b ** (p - 1), c * kappa * p * (p - 1) * b ** (p - 2)
			E = xs[None, :, :].expand(a.shape[0], -1, -1)
			diag = torch.zeros_like(w1)
		else:
			E = a[:, None, :] - xs[None, :, :]
			r2 = (E * E).sum(-1)
			if kind == 0:
				e = kappa * torch.exp(-0.5 * r2)
				w1, w2 = -c * e, c * e
			else:
				r = torch.sqrt(r2)
				e = kappa * torch.exp(-SQ5 * r)
				w1, w2 = -c * (5.0 / 3.0) * (1 + SQ5 * r) * e, c * (25.0 / 3.0) * e
			diag = w1
		out.append(torch.einsum("mi,mik->mk", w1, E) * il)
		if hess:
			h = torch.einsum("mi,mia,mib->mab", w2, E, E) + torch.diag_embed(diag.sum(1)[:, None].expand(-1, x.shape[1]))
			outh.append(h * il[:, None] * il[None, :])
	return torch.cat(out), (torch.cat(outh) if hess else None)


def _dev_grad(kind, x, xt, il, kappa, offset, alpha, u, Wt, v, order=1):
	from stpy_amd import _lib as L
	lib = L.load()
	m, n, d = xt.shape[0], x.shape[0], x.shape[1]
	dt = L.dtype_code(x.dtype)
	G = torch.full((m, d), float("nan"), dtype=x.dtype, device=x.device)
	H = torch.full((m, d, d), float("nan"), dtype=x.dtype, device=x.device) if order == 2 else None
	work = torch.empty((int(lib.stpy_gram_grad_workspace_bytes(dt, m, n, d, order)),), dtype=torch.uint8, device=x.device)
	L.check(lib.stpy_gram_grad(kind, dt, L.ptr(x), n, x.stride(0), L.ptr(xt), m, xt.stride(0), d, None, L.ptr(il), kappa, offset,
							   L.ptr(alpha), L.ptr(u), L.ptr(Wt), Wt.stride(0) if Wt is not None else 0, L.ptr(v), order, 0,
							   L.ptr(G), G.stride(0), L.ptr(H), L.ptr(work), work.numel(), L.stream_ptr()), "stpy_gram_grad")
	return G, H


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 127, 1000, 8000])
@pytest.mark.parametrize("M", [1, 300, 1000])
@pytest.mark.parametrize("d", [1, 3, 16, 40])
def test_gpu_gram_grad_ragged(gpu_device, N, M, d):
	gen = torch.Generator(device="cpu").manual_seed(N * 1000003 + M * 101 + d)
	x = torch.rand((N, d), generator=gen, dtype=torch.float64).to(gpu_device) * 2 - 1
	xt = torch.rand((M, d), generator=gen, dtype=torch.float64).to(gpu_device) * 2 - 1
	il = (0.5 + torch.rand(d, generator=gen, dtype=torch.float64) * 2 / np.sqrt(d)).to(gpu_device)
	alpha = torch.randn(N, generator=gen, dtype=torch.float64).to(gpu_device)
	u = torch.randn(M, generator=gen, dtype=torch.float64).to(gpu_device)
	v = torch.randn(M, generator=gen, dtype=torch.float64).to(gpu_device)
	Wt = torch.randn((M, N + 5), generator=gen, dtype=torch.float64).to(gpu_device)        # ldw > n
	kinds = [(0, 1.3, 0.0), (3, 0.8, 0.0), (5 | (3 << 8), 0.2, 1.0)]
	for kind, kappa, offset in kinds:
		G, _ = _dev_grad(kind, x, xt, il, kappa, offset, alpha, u, Wt, v)
		G2, _ = _dev_grad(kind, x, xt, il, kappa, offset, alpha, u, Wt, v)
		assert torch.equal(G, G2), "two calls differ"
		R, _ = _torch_grad(kind, x, xt, il, kappa, offset, alpha, u, Wt, v)
		assert rel_err(G.cpu().numpy(), R.cpu().numpy()) < 1e-11, (kind, N, M, d)
	# coefficient halves alone (NULL alpha / NULL Wt, NULL scales)
	G, _ = _dev_grad(0, x, xt, il, 1.0, 0.0, None, None, Wt, None)
	R, _ = _torch_grad(0, x, xt, il, 1.0, 0.0, None, None, Wt, torch.ones(M, dtype=torch.float64, device=gpu_device))
	assert rel_err(G.cpu().numpy(), R.cpu().numpy()) < 1e-11
	if M == 1:
		for kind, kappa, offset in kinds:
			G, H = _dev_grad(kind, x, xt, il, kappa, offset, alpha, u, None, None, order=2)
			R, RH = _torch_grad(kind, x, xt, il, kappa, offset, alpha, u, None, None, hess=True)
			assert rel_err(G.cpu().numpy(), R.cpu().numpy()) < 1e-11
			assert rel_err(H.cpu().numpy(), RH.cpu().numpy()) < 1e-11
	if N == 1000 and d in (3, 16):                    # fp32 within 1e-3 of fp64
		f = lambda t: None if t is None else t.float()
		for kind, kappa, offset in kinds:
			G64, _ = _dev_grad(kind, x, xt, il, kappa, offset, alpha, u, Wt, v)
			G32, _ = _dev_grad(kind, f(x), f(xt), f(il), kappa, offset, f(alpha), f(u), f(Wt), f(v))
			assert rel_err(G32.double().cpu().numpy(), G64.cpu().numpy()) < 1e-3


@pytest.mark.gpu
def test_gpu_gp_fp32_close_to_fp64(gpu_device):
	g = golden("G17_posterior_grad")
	k = make_kernel(CASES["ard_groups"])
	d64 = _gp(k, g["x"], g["y"]).mean_std_grad(torch.from_numpy(g["xb"]))
	d32 = _gp(make_kernel(CASES["ard_groups"]), g["x"], g["y"], dtype=torch.float32).mean_std_grad(torch.from_numpy(g["xb"]).float())
	for a, b in zip(d32, d64):
		assert a.dtype == torch.float32 and rel_err(a.double().numpy(), b.numpy()) < 1e-3


def _factor(n0, dtype, dev, seed):
	"""Tile-padded Cholesky factor (identity border, as GaussianProcess holds it) of a well-conditioned SPD matrix."""
	from stpy_amd import _lib as L
	lib = L.load()
	n = -(-n0 // 128) * 128
	gen = torch.Generator(device="cpu").manual_seed(seed)
	R = torch.randn((n0, n0), generator=gen, dtype=torch.float64)
	A = torch.eye(n, dtype=torch.float64)
	A[:n0, :n0] = R @ R.T / n0 + torch.eye(n0, dtype=torch.float64)
	A = A.to(device=dev, dtype=dtype)
	dt = L.dtype_code(dtype)
	winv = torch.empty((int(lib.stpy_potrf_winv_elems(n)),), dtype=dtype, device=dev)
	work = torch.empty((int(lib.stpy_potrf_workspace_bytes(dt, n, 0)),), dtype=torch.uint8, device=dev)
	info = torch.zeros((1,), dtype=torch.int32, device=dev)
	L.check(lib.stpy_potrf(dt, n, L.ptr(A), n, L.ptr(winv), winv.numel(), L.ptr(work), work.numel(), 0, 0, L.ptr(info), L.stream_ptr()), "stpy_potrf")
	assert int(info.item()) == 0
	return A, winv


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 1e-4)])
@pytest.mark.parametrize("n0", [128, 1000, 4096])
def test_gpu_trsm_right_ln(gpu_device, dtype, tol, n0):
	from stpy_amd import _lib as L
	lib = L.load()
	A, winv = _factor(n0, dtype, gpu_device, n0)
	n = A.shape[0]
	dt = L.dtype_code(dtype)
	Lr = torch.empty_like(A)
	winvr = torch.empty_like(winv)
	L.check(lib.stpy_trsm_ln_factor(dt, n, L.ptr(A), n, L.ptr(winv), winv.numel(), L.ptr(Lr), n, L.ptr(winvr), L.stream_ptr()), "stpy_trsm_ln_factor")
	Lt = torch.tril(A)
	for m in (1, 7, 300, 2048):
		B = torch.randn((m, n), dtype=torch.float64, device=gpu_device).to(dtype)
		X = B.clone()
		tw = torch.empty((int(lib.stpy_trsm_workspace_bytes(dt, m, n, 0)),), dtype=torch.uint8, device=gpu_device)
		L.check(lib.stpy_trsm_right_ln(dt, m, n, L.ptr(Lr), n, L.ptr(winvr), winvr.numel(), L.ptr(X), n, 0, 0, L.ptr(tw), tw.numel(), L.stream_ptr()),
				"stpy_trsm_right_ln")
		assert rel_err((X.double() @ Lt.double()).cpu().numpy(), B.double().cpu().numpy()) < tol
		ref = torch.linalg.solve_triangular(Lt.double(), B.double(), upper=False, left=False)
		assert rel_err(X.double().cpu().numpy(), ref.cpu().numpy()) < tol


def _ucb_problem(d, seed):
	from stpy_amd import GaussianProcess
	rng = np.random.RandomState(seed)
	x = rng.uniform(-1, 1, size=(25, d))
	y = np.sin(3 * x[:, :1]) * np.cos(2 * x[:, -1:]) + 0.05 * rng.normal(size=(25, 1))
	GP = GaussianProcess(gamma=0.4, s=0.05, kappa=1.0, d=d, bounds=[(-1.0, 1.0)] * d)
	GP.fit_gp(torch.from_numpy(x), torch.from_numpy(y))
	return GP


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 2])
def test_gpu_ucb_optimize(gpu_device, d):
	GP = _ucb_problem(d, 7 + d)
	beta = 2.0
	np.random.seed(3)
	sol, val = GP.ucb_optimize(beta, multistart=10)
	s = sol.numpy()
	assert s.shape == (d,) and np.all(s >= -1.0) and np.all(s <= 1.0)
	mu, sd = GP.mean_std(torch.from_numpy(s.reshape(1, d)))
	assert abs(float(val) - float(mu + np.sqrt(beta) * sd)) < 1e-10
	grid = np.stack(np.meshgrid(*[np.linspace(-1, 1, 401 if d == 1 else 201)] * d, indexing="ij"), -1).reshape(-1, d)
	gm, gs = GP.mean_std(torch.from_numpy(grid))
	assert float(val) >= float((gm + np.sqrt(beta) * gs).max()) - 1e-6
	dmu, dstd = GP.mean_std_grad(torch.from_numpy(s.reshape(1, d)))
	g = (dmu + np.sqrt(beta) * dstd).numpy().reshape(-1)
	proj = np.clip(s + g, -1.0, 1.0) - s                        # projected gradient of the maximisation
	assert np.abs(proj).max() <= 1e-5
	np.random.seed(3)
	sol_l, val_l = GP.ucb_optimize(beta, multistart=10, lcb=True)
	mu, sd = GP.mean_std(torch.from_numpy(sol_l.numpy().reshape(1, d)))
	assert abs(float(val_l) - float(mu - np.sqrt(beta) * sd)) < 1e-10
	assert float(val_l) >= float((gm - np.sqrt(beta) * gs).max()) - 1e-6
	GP.bounds = None
	with pytest.raises(ValueError):
		GP.ucb_optimize(beta)


@pytest.mark.gpu
def test_gpu_not_implemented_paths(gpu_device):
	from stpy_amd import RFFEmbedding
	from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures
	g = golden("G17_posterior_grad")
	GP = _gp(make_kernel(CASES["se"]), g["x"], g["y"])
	with pytest.raises(NotImplementedError, match="get_2_der"):
		GP.gradient_mean_var(torch.from_numpy(g["pts"][:1]), hessian=True)
	with pytest.raises(ValueError):
		GP.mean_std(torch.from_numpy(g["xb"]).requires_grad_(True), full=True)
	emb = RFFEmbedding(gamma=0.7, m=32, d=D)
	KF = KernelizedFeatures(embedding=emb, m=32, d=D)
	KF.fit_gp(torch.from_numpy(g["x"]), torch.from_numpy(g["y"]))
	for call in (lambda: KF.mean_std_grad(torch.from_numpy(g["xb"])), lambda: KF.mean_gradient_hessian(torch.from_numpy(g["pts"][:1])),
				 lambda: KF.gradient_mean_var(torch.from_numpy(g["pts"][:1])), lambda: KF.ucb_optimize(2.0)):
		with pytest.raises(NotImplementedError, match="KernelizedFeatures"):
			call()


@pytest.mark.gpu
def test_gpu_unfitted_prior_and_chunks(gpu_device):
	from stpy_amd import GaussianProcess
	g = golden("G17_posterior_grad")
	for spec in (CASES["se_plus_linear"], CASES["poly"]):
		k = make_kernel(spec)
		GP = GaussianProcess(kernel=k, s=0.1, d=D)
		xb = g["xb"]
		xt = torch.from_numpy(xb).requires_grad_(True)
		mu, sd = GP.mean_std(xt)
		(mu.sum() + sd.sum()).backward()
		kd = np.array([kernel_kgh(k, xb[i:i + 1], xb[i:i + 1])[0][0, 0] for i in range(len(xb))])
		gself = np.stack([2.0 * kernel_kgh(k, xb[i:i + 1], xb[i:i + 1])[1][0, 0] for i in range(len(xb))])
		assert rel_err(xt.grad.numpy(), gself / (2.0 * np.sqrt(kd))[:, None]) < 1e-10
	# chunked prediction (max_size) gives the same gradient as one chunk
	GP = _gp(make_kernel(CASES["se_plus_linear"]), g["x"], g["y"])
	xt = torch.from_numpy(g["xb"]).requires_grad_(True)
	GP.mean_std(xt)[1].sum().backward()
	full = xt.grad.clone()
	GP.max_size = 4
	xt.grad = None
	GP.mean_std(xt)[1].sum().backward()
	assert rel_err(xt.grad.numpy(), full.numpy()) < 1e-13
