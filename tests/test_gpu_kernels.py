"""
GPU parity tests of the individual C-ABI entry points (include/stpy_hip.h) against the CPU oracle /
numpy on the same seeded inputs.  Run with `-m gpu` on an MI355X.
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from oracle import gp_oracle as O
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

TOL64 = 1e-11


@pytest.fixture(scope="module")
def L(gpu_device):
	from stpy_amd import _lib
	return _lib


def dev(a, dtype=torch.float64):
	return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda:0", dtype=dtype)


def spd(rng, n, d=4, s=0.3):
	x = rng.uniform(-1, 1, size=(n, d))
	return O.gram_train(x, [("squared_exponential", {"gamma": 1.0, "kappa": 1.0}, "-")], s)


# ------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("n,k,lda_pad", [(2048, 64, 0), (2176, 288, 4), (4096, 1056, 0), (2304, 32 * 37, 12), (2048, 16384, 0), (2304, 8192 + 32 * 5, 4)])
def test_syrk_from_planes_is_bit_identical_to_gemm_nt(L, n, k, lda_pad):
	"""stpy_syrk with its workspace (fp32: A split once into tile-major bf16 planes, gemm_bf3p.hip) against stpy_gemm_nt(A, A, lower_only)
	(every tile splits on the fly): all three modes, bit for bit on the lower tiles; and against an fp64 product.  The last two shapes
	(few tiles, long K) cut K into chunks for the modes that may (0 and 2; the workspace query then asks for the chunk buffers): there the two
	routes group the same partial sums differently -- agreement to fp32 rounding instead of bit for bit, and the same bits on every run."""
	lib = L.load()
	torch.manual_seed(n + k)
	lda = k + lda_pad
	Abuf = torch.randn(n, lda, dtype=torch.float32, device="cuda:0")
	A = Abuf[:, :k]
	wb = int(lib.stpy_syrk_workspace_bytes(L.F32, n, k))
	nbuf = (wb - 3 * n * k * 2) // (n * n * 4)
	assert wb == 3 * n * k * 2 + nbuf * n * n * 4 and (nbuf > 0) == (k >= 8192)
	work = torch.empty(wb, dtype=torch.uint8, device="cuda:0")
	C0 = torch.randn(n, n, dtype=torch.float32, device="cuda:0")
	low = torch.ones(n // 128, n // 128, device="cuda:0").tril().bool().repeat_interleave(128, 0).repeat_interleave(128, 1)      # the lower 128 x 128 tiles
	ref64 = A.double() @ A.double().T
	for mode in (0, 1, 2):
		Ca, Cb = C0.clone(), C0.clone()
		# (the comparison is with the on-the-fly bf16 split: the few-tile sliver route, which would take these small products onto the fp32 MFMA, is off)
		keep30 = int(lib.stpy_tune_get(30))
		lib.stpy_tune(30, 0)
		try:
			L.check(lib.stpy_gemm_nt(L.F32, n, n, k, L.ptr(A), lda, L.ptr(A), lda, L.ptr(Ca), n, mode, 1, L.stream_ptr()), "gemm")
		finally:
			lib.stpy_tune(30, keep30)
		L.check(lib.stpy_syrk(L.F32, n, k, L.ptr(A), lda, L.ptr(Cb), n, mode, L.ptr(work), wb, L.stream_ptr()), "syrk")
		torch.cuda.synchronize()
		if nbuf == 0 or mode == 1:
			assert torch.equal(Ca[low], Cb[low]), mode
		else:
			assert float((Ca - Cb)[low].abs().max()) < 2e-6 * float(Ca[low].abs().max()), mode          # (a few ulps of the largest sums: 128 chunk-level additions each)
			Cr = C0.clone()
			L.check(lib.stpy_syrk(L.F32, n, k, L.ptr(A), lda, L.ptr(Cr), n, mode, L.ptr(work), wb, L.stream_ptr()), "syrk")
			assert torch.equal(Cr, Cb), mode                        # the chunk sums are added in index order: reproducible
		assert torch.equal(Cb[~low], C0[~low])                    # tiles above the diagonal untouched
		want = {0: ref64, 1: C0.double() - ref64, 2: C0.double() + ref64}[mode]
		assert float((Cb.double() - want)[low].abs().max()) < 2e-5 * float(want.abs().max())
	# without a workspace, in fp64, or for a shape the route does not take: the plain product
	Cc = C0.clone()
	L.check(lib.stpy_syrk(L.F32, n, k, L.ptr(A), lda, L.ptr(Cc), n, 1, None, 0, L.stream_ptr()), "syrk")
	Cd = C0.clone()
	L.check(lib.stpy_gemm_nt(L.F32, n, n, k, L.ptr(A), lda, L.ptr(A), lda, L.ptr(Cd), n, 1, 1, L.stream_ptr()), "gemm")
	assert torch.equal(Cc[low], Cd[low])                          # (same routing rules for both entry points)
	assert int(lib.stpy_syrk_workspace_bytes(L.F64, n, k)) == 0 and int(lib.stpy_syrk_workspace_bytes(L.F32, 1920, k)) == 0
	A64 = torch.randn(300, 70, dtype=torch.float64, device="cuda:0")
	C64 = torch.zeros(300, 300, dtype=torch.float64, device="cuda:0")
	L.check(lib.stpy_syrk(L.F64, 300, 70, L.ptr(A64), 70, L.ptr(C64), 300, 0, None, 0, L.stream_ptr()), "syrk")
	assert rel_err(np.tril(C64.cpu().numpy()), np.tril((A64 @ A64.T).cpu().numpy())) < 1e-14


@pytest.mark.parametrize("m,n,k", [(128, 128, 16), (256, 384, 128), (300, 200, 70), (1, 130, 5), (513, 129, 257), (1024, 1024, 512)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gemm_nt(L, m, n, k, mode):
	rng = np.random.RandomState(m * 7 + n * 3 + k + mode)
	A, B, C = rng.normal(size=(m, k)), rng.normal(size=(n, k)), rng.normal(size=(m, n))
	Ad, Bd, Cd = dev(A), dev(B), dev(C)
	lib = L.load()
	rc = lib.stpy_gemm_nt(L.F64, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd), n, mode, 0, L.stream_ptr())
	L.check(rc, "gemm")
	ref = A @ B.T if mode == 0 else (C - A @ B.T if mode == 1 else C + A @ B.T)
	assert rel_err(Cd.cpu().numpy(), ref) < 1e-14 * max(1, k) ** 0.5 * 10
	assert lib.stpy_gemm_nt(L.F64, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd), n, 3, 0, L.stream_ptr()) == -11          # unknown mode: refused


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-13), (torch.float32, 2e-5)])
def test_gemm_nt_accumulate_lower(L, dtype, tol):
	"""mode 2 (C += A B^T) on the lower tiles of a square C, slab after slab: what KernelizedFeatures.fit_gp does with Phi^T Phi.
	Aligned slabs take the direct-to-VGPR kernel, the ragged last one the guarded tile kernel; the upper tiles are never touched."""
	lib = L.load()
	rng = np.random.RandomState(17)
	m, slabs = 512, (1024, 768, 333)
	code = L.dtype_code(dtype)
	npdt = np.float64 if dtype == torch.float64 else np.float32
	Cd = torch.full((m, m), float("nan"), dtype=dtype, device="cuda:0")
	ref = np.zeros((m, m))
	for i, k in enumerate(slabs):
		A = rng.normal(size=(m, k)).astype(npdt)
		Ad = dev(A, dtype)
		L.check(lib.stpy_gemm_nt(code, m, m, k, L.ptr(Ad), k, L.ptr(Ad), k, L.ptr(Cd), m, 0 if i == 0 else 2, 1, L.stream_ptr()), "gemm")
		ref += A.astype(np.float64) @ A.astype(np.float64).T
	got = Cd.cpu().numpy().astype(np.float64)
	tiles = np.arange(m) // 128
	low = tiles[:, None] >= tiles[None, :]
	assert rel_err(got[low], ref[low]) < tol
	assert np.isnan(got[~low]).all()


@pytest.mark.parametrize("m,n,k,lower", [(1024, 1024, 512, 0), (2048, 512, 1024, 0), (1536, 1536, 256, 1), (1024, 1024, 64, 0), (1024, 1024, 8192, 0)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gemm_nt_f32_on_bf16_matrix_cores(L, m, n, k, lower, mode):
	"""Aligned fp32 products of >= 64 tiles run on the bf16 matrix cores from an EXACT three-way split of both operands (six
	products, fp32 accumulation; stpy_tune route key 26, 0 = the fp32-MFMA kernels).  Against fp64 numpy the result must be as
	accurate as the fp32-MFMA kernel's, on data that stresses the split: six decades of dynamic range inside a row, exact zeros,
	mixed signs, values with all 24 significand bits set.  K = 8192 is the long-accumulation case: the bf16 MFMA's accumulate is not
	round-to-nearest (half an ulp of the accumulator lost per instruction, toward zero), which is why the kernel carries only
	128-deep partial sums in the MFMA accumulator and adds them on the vector ALU -- without that this case fails by 4-5x."""
	lib = L.load()
	rng = np.random.RandomState(m + n + k + 7 * mode + lower)
	def stress(shape):
		a = rng.normal(size=shape) * 10.0 ** rng.uniform(-3, 3, size=shape)
		a[rng.uniform(size=shape) < 0.05] = 0.0
		a = a.astype(np.float32)
		a.view(np.uint32)[::7, ::5] |= np.uint32(0x007fffff)          # full significands
		return a
	A, B, C = stress((m, k)), stress((n, k)), (rng.normal(size=(m, n)) * 1e3).astype(np.float32)
	ref64 = A.astype(np.float64) @ B.astype(np.float64).T
	ref = ref64 if mode == 0 else (C.astype(np.float64) - ref64 if mode == 1 else C.astype(np.float64) + ref64)
	scale = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T + np.abs(C) * (mode != 0)          # elementwise error scale
	outs = {}
	assert lib.stpy_tune_get(26) > 0
	try:
		for route in (lib.stpy_tune_get(26), 0):
			lib.stpy_tune(26, route)
			Ad, Bd, Cd = dev(A, torch.float32), dev(B, torch.float32), dev(C, torch.float32)
			L.check(lib.stpy_gemm_nt(L.F32, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd), n, mode, lower, L.stream_ptr()), "gemm")
			outs[route] = Cd.cpu().numpy().astype(np.float64)
	finally:
		lib.stpy_tune(26, 64)
	tiles = np.arange(m)[:, None] // 128 >= np.arange(n)[None, :] // 128 if lower else np.ones((m, n), bool)
	errs = {r: float(np.max(np.abs(o - ref)[tiles] / scale[tiles])) for r, o in outs.items()}
	bf3, f32 = errs[[r for r in errs if r][0]], errs[0]
	assert bf3 < 4e-6 and bf3 <= 2.0 * f32 + 1e-7, errs
	if lower:          # tiles above the diagonal untouched
		for o in outs.values():
			assert np.array_equal(o[~tiles], C.astype(np.float64)[~tiles])


@pytest.mark.parametrize("m,n,k,mode", [(1, 512, 4096, 0), (1, 300, 1001, 1), (2, 128, 640, 0), (3, 257, 96, 1), (5, 64, 2048, 0), (8, 512, 1536, 1)])
def test_gemm_nt_skinny_rows(L, m, n, k, mode):
	"""m <= 8 goes to the bandwidth-bound row kernel (z = L^-1 y on the distributed path)."""
	rng = np.random.RandomState(m * 11 + n + k)
	A, B, C = rng.normal(size=(m, k)), rng.normal(size=(n, k)), rng.normal(size=(m, n))
	Ad, Bd, Cd = dev(A), dev(B), dev(C)
	lib = L.load()
	L.check(lib.stpy_gemm_nt(L.F64, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd), n, mode, 0, L.stream_ptr()), "gemm")
	ref = A @ B.T if mode == 0 else C - A @ B.T
	assert rel_err(Cd.cpu().numpy(), ref) < 1e-13
	Cd2 = dev(C)
	L.check(lib.stpy_gemm_nt(L.F64, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd2), n, 2, 0, L.stream_ptr()), "gemm")
	assert rel_err(Cd2.cpu().numpy(), C + A @ B.T) < 1e-13


@pytest.mark.parametrize("m,n,k,mode,passes", [(256, 128, 4096, 0, 4), (512, 256, 3000, 1, 3), (130, 100, 2500, 0, 5), (128, 128, 1024, 1, 16)])
def test_gemm_nt_splitk(L, m, n, k, mode, passes):
	rng = np.random.RandomState(m + n + k + passes)
	A, B, C = rng.normal(size=(m, k)), rng.normal(size=(n, k)), rng.normal(size=(m, n))
	Ad, Bd, Cd = dev(A), dev(B), dev(C)
	work = torch.full((passes * m * n,), float("nan"), dtype=torch.float64, device="cuda:0")
	lib = L.load()
	L.check(lib.stpy_gemm_nt_splitk(L.F64, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd), n, mode, passes, L.ptr(work), work.numel() * work.element_size(), L.stream_ptr()), "splitk")
	ref = A @ B.T if mode == 0 else C - A @ B.T
	assert rel_err(Cd.cpu().numpy(), ref) < 1e-13
	# the same call twice gives the same bits (fixed summation order)
	Cd2 = dev(C)
	L.check(lib.stpy_gemm_nt_splitk(L.F64, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd2), n, mode, passes, L.ptr(work), work.numel() * work.element_size(), L.stream_ptr()), "splitk")
	assert torch.equal(Cd, Cd2)


def test_gemm_nt_splitk_plan(L):
	lib = L.load()
	assert lib.stpy_gemm_nt_splitk_passes(4096, 512, 32768) >= 2        # 128 tiles, long K
	assert lib.stpy_gemm_nt_splitk_passes(4096, 512, 512) == 1          # short K
	assert lib.stpy_gemm_nt_splitk_passes(8192, 8192, 65536) == 1       # plenty of tiles
	assert lib.stpy_gemm_nt_splitk_passes(1, 512, 65536) == 1           # row kernel instead
	assert lib.stpy_gemm_nt_splitk(L.F64, 256, 256, 4096, 1, 4096, 1, 4096, 1, 256, 0, 4, None, 0, None) != 0
	assert b"workspace" in lib.stpy_last_error_string()


@pytest.mark.parametrize("m,n,mode", [(300, 128, 0), (4096, 128, 1), (1000, 256, 1), (64, 128, 0), (129, 384, 0)])
def test_gemm_nt_k128_small_grid(L, m, n, mode):
	"""K = 128 on a small grid takes the one-volley kernel (panel chain); also in place, C aliasing A (n = k = 128)."""
	rng = np.random.RandomState(m + n + mode)
	k = 128
	A, B, C = rng.normal(size=(m, k)), rng.normal(size=(n, k)), rng.normal(size=(m, n))
	Ad, Bd, Cd = dev(A), dev(B), dev(C)
	lib = L.load()
	L.check(lib.stpy_gemm_nt(L.F64, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd), n, mode, 0, L.stream_ptr()), "gemm")
	ref = A @ B.T if mode == 0 else C - A @ B.T
	assert rel_err(Cd.cpu().numpy(), ref) < 1e-13
	Cd2 = dev(C)
	L.check(lib.stpy_gemm_nt(L.F64, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd2), n, 2, 0, L.stream_ptr()), "gemm")
	assert rel_err(Cd2.cpu().numpy(), C + A @ B.T) < 1e-13
	# the same product with the kernel switched off gives the same numbers to rounding
	lib.stpy_tune(8, 0)
	try:
		Cd2 = dev(C)
		L.check(lib.stpy_gemm_nt(L.F64, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd2), n, mode, 0, L.stream_ptr()), "gemm")
	finally:
		lib.stpy_tune(8, 768)
	assert rel_err(Cd2.cpu().numpy(), ref) < 1e-13
	if n == 128 and mode == 0:        # in place: A <- A B^T inside a wider buffer (the block solve's multiply by an inverse block)
		big = rng.normal(size=(m, 400))
		bd = dev(big)
		pa = ctypes.c_void_p(bd.data_ptr() + 128 * 8)
		L.check(lib.stpy_gemm_nt(L.F64, m, 128, 128, pa, 400, L.ptr(Bd), k, pa, 400, 0, 0, L.stream_ptr()), "gemm")
		out = bd.cpu().numpy()
		assert rel_err(out[:, 128:256], big[:, 128:256] @ B.T) < 1e-13
		assert np.array_equal(out[:, :128], big[:, :128]) and np.array_equal(out[:, 256:], big[:, 256:])


def test_undersized_workspace_is_refused(L):
	"""a workspace smaller than the query's answer comes back as error -20, not as a write past its end"""
	lib = L.load()
	n = 1024
	Kd = dev(np.eye(n) * 2.0)
	winv = torch.empty(int(lib.stpy_potrf_winv_elems(n)), dtype=torch.float64, device="cuda:0")
	info = torch.zeros(1, dtype=torch.int32, device="cuda:0")
	small = torch.empty(int(lib.stpy_potrf_workspace_bytes(L.F64, n, 256)), dtype=torch.uint8, device="cuda:0")
	assert lib.stpy_potrf(L.F64, n, L.ptr(Kd), n, L.ptr(winv), winv.numel(), L.ptr(small), small.numel(), 512, 0, L.ptr(info), L.stream_ptr()) == -20
	assert b"workspace" in lib.stpy_last_error_string()
	assert lib.stpy_potrf(L.F64, n, L.ptr(Kd), n, L.ptr(winv), winv.numel(), L.ptr(small), small.numel(), 256, 0, L.ptr(info), L.stream_ptr()) == 0
	x = dev(np.random.RandomState(0).normal(size=(300, 5)))
	il = dev(np.ones(5))
	out = torch.empty((300, 300), dtype=torch.float64, device="cuda:0")
	tiny = torch.empty(64, dtype=torch.uint8, device="cuda:0")
	assert lib.stpy_gram(0, L.F64, L.ptr(x), 300, 5, L.ptr(x), 300, 5, 5, None, L.ptr(il), 1.0, 0.0, 0.0, 0, 0, L.ptr(out), 300, L.ptr(tiny), 64, L.stream_ptr()) == -20
	torch.cuda.synchronize()


def test_undersized_winv_is_refused(L):
	"""every entry point that takes the inverse diagonal blocks takes their element count and refuses a short array (-21)"""
	lib = L.load()
	n = 1024
	Kd = dev(np.eye(n) * 2.0)
	need = int(lib.stpy_potrf_winv_elems(n))
	assert need == (n // 128) * 128 * 128
	short = torch.empty(need - 128 * 128, dtype=torch.float64, device="cuda:0")
	winv = torch.empty(need, dtype=torch.float64, device="cuda:0")
	info = torch.zeros(1, dtype=torch.int32, device="cuda:0")
	work = torch.empty(int(lib.stpy_potrf_workspace_bytes(L.F64, n, 0)), dtype=torch.uint8, device="cuda:0")
	assert lib.stpy_potrf(L.F64, n, L.ptr(Kd), n, L.ptr(short), short.numel(), L.ptr(work), work.numel(), 0, 0, L.ptr(info), L.stream_ptr()) == -21
	assert b"winv" in lib.stpy_last_error_string()
	assert lib.stpy_potrf(L.F64, n, L.ptr(Kd), n, L.ptr(winv), winv.numel(), L.ptr(work), work.numel(), 0, 0, L.ptr(info), L.stream_ptr()) == 0
	B = dev(np.ones((256, n)))
	assert lib.stpy_trsm_right_lt(L.F64, 256, n, L.ptr(Kd), n, L.ptr(winv), short.numel(), L.ptr(B), n, 0, 0, None, 0, L.stream_ptr()) == -21
	y, z = dev(np.ones(n)), dev(np.zeros(n))
	assert lib.stpy_trsv(L.F64, n, L.ptr(Kd), n, L.ptr(winv), short.numel(), L.ptr(y), L.ptr(z), 0, L.stream_ptr()) == -21
	Kinv = torch.empty((n, n), dtype=torch.float64, device="cuda:0")
	w2 = torch.empty((n, n), dtype=torch.float64, device="cuda:0")
	assert lib.stpy_potri(L.F64, n, L.ptr(Kd), n, L.ptr(winv), short.numel(), L.ptr(Kinv), n, L.ptr(w2), w2.numel() * 8, L.stream_ptr()) == -21
	# unknown flag bits are refused too
	assert lib.stpy_potrf(L.F64, n, L.ptr(Kd), n, L.ptr(winv), winv.numel(), L.ptr(work), work.numel(), 0, 64, L.ptr(info), L.stream_ptr()) == -10
	torch.cuda.synchronize()


def test_two_threads_two_streams(L):
	"""Two host threads factor and solve two different SPD systems concurrently, each on its own HIP stream.  The look-ahead
	side stream and events are per caller stream, the error string is thread-local and the per-call behaviour is a flag,
	so the results are identical (bit for bit) to the same calls issued one after the other."""
	import threading
	lib = L.load()
	n, m = 4096, 1024
	rng = np.random.RandomState(11)
	mats = []
	for t in range(2):
		A = rng.normal(size=(n, 64))
		K = A @ A.T / 64.0 + (2.0 + t) * np.eye(n)
		mats.append((K, rng.normal(size=(m, n))))

	def run(K, B, stream, flags):
		with torch.cuda.stream(stream):
			Kd, Bd = dev(K), dev(B)
			winv = torch.empty(int(lib.stpy_potrf_winv_elems(n)), dtype=torch.float64, device="cuda:0")
			work = torch.empty(int(lib.stpy_potrf_workspace_bytes(L.F64, n, 0)), dtype=torch.uint8, device="cuda:0")
			info = torch.zeros(1, dtype=torch.int32, device="cuda:0")
			sp = ctypes.c_void_p(stream.cuda_stream)
			for _ in range(3):          # several calls per thread: the two threads' launches interleave
				Kd.copy_(dev(K))
				Bd.copy_(dev(B))
				assert lib.stpy_potrf(L.F64, n, L.ptr(Kd), n, L.ptr(winv), winv.numel(), L.ptr(work), work.numel(), 0, flags, L.ptr(info), sp) == 0
				assert lib.stpy_trsm_right_lt(L.F64, m, n, L.ptr(Kd), n, L.ptr(winv), winv.numel(), L.ptr(Bd), n, 0, flags, None, 0, sp) == 0
			stream.synchronize()
			assert int(info.item()) == 0
			return torch.tril(Kd).cpu().numpy(), Bd.cpu().numpy()

	torch.cuda.synchronize()
	s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
	serial = [run(mats[0][0], mats[0][1], s0, 0), run(mats[1][0], mats[1][1], s1, L.FLAG_BESIDE_UPDATE)]
	out = [None, None]
	errs = []

	def worker(i, stream, flags):
		try:
			torch.cuda.set_device(0)
			out[i] = run(mats[i][0], mats[i][1], stream, flags)
		except Exception as exc:          # noqa: BLE001
			errs.append(exc)
	th = [threading.Thread(target=worker, args=(0, s0, 0)), threading.Thread(target=worker, args=(1, s1, L.FLAG_BESIDE_UPDATE))]
	for t in th:
		t.start()
	for t in th:
		t.join()
	assert not errs, errs
	for i in range(2):
		assert np.array_equal(out[i][0], serial[i][0]) and np.array_equal(out[i][1], serial[i][1])
		Lf = np.linalg.cholesky(mats[i][0])
		assert rel_err(out[i][0], Lf) < 1e-12
		assert rel_err(out[i][1], np.linalg.solve(Lf, mats[i][1].T).T) < 1e-11


@pytest.mark.parametrize("m,n,k,nbd,pr,pc,myr,myc,i0,j0", [
	(1024, 768, 256, 256, 2, 2, 1, 0, 1, 0),        # aligned: direct-to-VGPR kernel with the staircase predicate
	(1024, 1024, 128, 128, 1, 4, 0, 2, 3, 0),
	(900, 640, 256, 128, 2, 4, 0, 3, 0, 1),         # ragged rows: guarded kernel
	(512, 512, 512, 512, 1, 1, 0, 0, 2, 2),         # one process: plain lower staircase at distribution-block granularity
])
def test_gemm_nt_bc_staircase(L, m, n, k, nbd, pr, pc, myr, myc, i0, j0):
	"""stpy_gemm_nt_bc: C -= A B^T on the 128x128 tiles whose distribution block (I, J) has I > J, and on the lower tiles of the
	diagonal blocks (I == J); all others untouched"""
	rng = np.random.RandomState(m + n + k + myr + myc)
	A, B, C = rng.normal(size=(m, k)), rng.normal(size=(n, k)), rng.normal(size=(m, n))
	Ad, Bd, Cd = dev(A), dev(B), dev(C)
	lib = L.load()
	L.check(lib.stpy_gemm_nt_bc(L.F64, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd), n, 1, nbd, pr, pc, myr, myc, i0, j0, L.stream_ptr()), "gemm_bc")
	out = Cd.cpu().numpy()
	full = C - A @ B.T
	nbt = nbd // 128
	for ti in range((m + 127) // 128):
		for tj in range((n + 127) // 128):
			I = (ti // nbt + i0) * pr + myr
			J = (tj // nbt + j0) * pc + myc
			blk = (slice(ti * 128, min(m, ti * 128 + 128)), slice(tj * 128, min(n, tj * 128 + 128)))
			if I > J or (I == J and tj % nbt <= ti % nbt):
				assert rel_err(out[blk], full[blk]) < 1e-13, (ti, tj)
			else:
				assert np.array_equal(out[blk], C[blk]), (ti, tj)


def test_gemm_nt_asymmetric_layout(L):
	"""A = I with an asymmetric B: catches a transposed C/D fragment map (cdna guide section 3)."""
	n = 128
	A = np.eye(n)
	B = np.arange(n * n, dtype=np.float64).reshape(n, n) / 7.0
	Ad, Bd, Cd = dev(A), dev(B), dev(np.zeros((n, n)))
	lib = L.load()
	L.check(lib.stpy_gemm_nt(L.F64, n, n, n, L.ptr(Ad), n, L.ptr(Bd), n, L.ptr(Cd), n, 0, 0, L.stream_ptr()), "gemm")
	assert np.array_equal(Cd.cpu().numpy(), B.T)


@pytest.mark.parametrize("n,k", [(512, 128), (1280, 512), (1000, 96)])
def test_gemm_nt_lower_only(L, n, k):
	rng = np.random.RandomState(n + k)
	P, C = rng.normal(size=(n, k)), rng.normal(size=(n, n))
	Pd, Cd = dev(P), dev(C)
	lib = L.load()
	L.check(lib.stpy_gemm_nt(L.F64, n, n, k, L.ptr(Pd), k, L.ptr(Pd), k, L.ptr(Cd), n, 1, 1, L.stream_ptr()), "gemm")
	out = Cd.cpu().numpy()
	ref = C - P @ P.T
	il = np.tril_indices(n)
	assert rel_err(out[il], ref[il]) < 1e-13
	# tiles strictly above the diagonal are untouched
	tiles = (n + 127) // 128
	for ti in range(tiles):
		for tj in range(ti + 1, tiles):
			blk = (slice(ti * 128, min(n, ti * 128 + 128)), slice(tj * 128, min(n, tj * 128 + 128)))
			assert np.array_equal(out[blk], C[blk])


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-13), (torch.float32, 3e-6)])
@pytest.mark.parametrize("m,n,k,lower,pad", [(1024, 1024, 256, 1, 0), (2048, 2048, 96 + 32, 1, 4), (640, 384, 64, 0, 0), (1536, 512, 1024, 0, 8), (3072, 3072, 512, 1, 0)])
def test_gemm_nt_few_tile_sliver_route(L, dtype, tol, m, n, k, lower, pad):
	"""Route key 30: plain / lower-only products of few 128 x 128 tiles run as 32 x 128 slivers (four times the workgroups), in fp64 and --
	round 4 -- in fp32 (fp32 MFMA, accumulating on -C when subtracting).  Both modes against an fp64 product, the route switched off against
	it switched on, operands inside padded buffers, tiles above the diagonal untouched."""
	lib = L.load()
	code = L.dtype_code(dtype)
	torch.manual_seed(m + n + k)
	Ab = torch.randn(m, k + pad, dtype=dtype, device="cuda:0")
	Bb = Ab if lower else torch.randn(n, k + pad, dtype=dtype, device="cuda:0")
	A, B = Ab[:, :k], Bb[:, :k]
	C0 = torch.randn(m, n + pad, dtype=dtype, device="cuda:0")
	ref = A.double() @ B.double().T
	keep = int(lib.stpy_tune_get(30))
	assert keep > 0
	outs = {}
	try:
		for route in (keep, 0):
			lib.stpy_tune(30, route)
			for mode in (0, 1):
				Cd = C0.clone()
				L.check(lib.stpy_gemm_nt(code, m, n, k, L.ptr(A), k + pad, L.ptr(B), k + pad, L.ptr(Cd), n + pad, mode, lower, L.stream_ptr()), "gemm")
				outs[(route, mode)] = Cd
	finally:
		lib.stpy_tune(30, keep)
	mask = torch.ones(m, n, dtype=torch.bool, device="cuda:0")
	if lower:
		mask = torch.ones(m // 128, n // 128, device="cuda:0").tril().bool().repeat_interleave(128, 0).repeat_interleave(128, 1)
	for mode in (0, 1):
		want = ref if mode == 0 else C0[:, :n].double() - ref
		for route in (keep, 0):
			got = outs[(route, mode)]
			assert float((got[:, :n].double() - want)[mask].abs().max()) < tol * float(want.abs().max()) * (k ** 0.5), (route, mode)
			assert torch.equal(got[:, :n][~mask], C0[:, :n][~mask]) and torch.equal(got[:, n:], C0[:, n:])


def test_gemm_nt_strided_submatrix(L):
	"""Leading dimensions larger than the logical width, operands inside bigger buffers."""
	rng = np.random.RandomState(5)
	big = rng.normal(size=(700, 900))
	bd = dev(big)
	m, n, k = 256, 128, 384
	A = big[128:128 + m, 256:256 + k]
	B = big[400:400 + n, 256:256 + k]
	C = rng.normal(size=(m, n))
	Cd = dev(C)
	lib = L.load()
	es = 8
	pa = ctypes.c_void_p(bd.data_ptr() + (128 * 900 + 256) * es)
	pb = ctypes.c_void_p(bd.data_ptr() + (400 * 900 + 256) * es)
	L.check(lib.stpy_gemm_nt(L.F64, m, n, k, pa, 900, pb, 900, L.ptr(Cd), n, 1, 0, L.stream_ptr()), "gemm")
	assert rel_err(Cd.cpu().numpy(), C - A @ B.T) < 1e-13


@pytest.mark.parametrize("m,n,k,mode", [(384, 256, 256, 0), (512, 512, 1024, 1), (256, 128, 64, 1), (1024, 384, 96, 0)])
def test_gemm_nt_f32_aligned(L, m, n, k, mode):
	"""fp32 on the tile-aligned paths (direct-to-VGPR kernel from k = 128, LDS-DMA kernel below; K tiles of 32 floats)"""
	rng = np.random.RandomState(m + n + k)
	A, B, C = [rng.normal(size=sh).astype(np.float32) for sh in ((m, k), (n, k), (m, n))]
	Ad, Bd, Cd = dev(A, torch.float32), dev(B, torch.float32), dev(C, torch.float32)
	lib = L.load()
	L.check(lib.stpy_gemm_nt(L.F32, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd), n, mode, 0, L.stream_ptr()), "gemm")
	P = A.astype(np.float64) @ B.astype(np.float64).T
	ref = P if mode == 0 else C.astype(np.float64) - P
	assert np.abs(Cd.cpu().numpy() - ref).max() < 2e-6 * np.sqrt(k) * max(1.0, np.abs(ref).max())


def test_gemm_nt_f32(L):
	rng = np.random.RandomState(9)
	m, n, k = 384, 256, 200
	A, B = rng.normal(size=(m, k)).astype(np.float32), rng.normal(size=(n, k)).astype(np.float32)
	Ad, Bd = dev(A, torch.float32), dev(B, torch.float32)
	Cd = torch.zeros((m, n), dtype=torch.float32, device="cuda:0")
	lib = L.load()
	L.check(lib.stpy_gemm_nt(L.F32, m, n, k, L.ptr(Ad), k, L.ptr(Bd), k, L.ptr(Cd), n, 0, 0, L.stream_ptr()), "gemm")
	assert rel_err(Cd.cpu().numpy(), A.astype(np.float64) @ B.astype(np.float64).T) < 5e-6


# ------------------------------------------------------------------------------------------ Gram
KINDS = [("se", 0), ("m12", 1), ("m32", 2), ("m52", 3), ("lin", 4)]


def oracle_gram(kind, a, b, inv_ls, kappa, offset, cols):
	ls = 1.0 / np.asarray(inv_ls)
	group = list(cols) if cols is not None else None
	if kind == 0:
		g = np.ones(a.shape[1]); g[group if group else slice(None)] = ls
		return O.ard(a, b, g, kappa, group)
	if kind in (1, 2, 3):
		g = np.ones(a.shape[1]); g[group if group else slice(None)] = ls
		aa, bb = a / g, b / g
		return O.matern(aa, bb, 1.0, {1: 0.5, 2: 1.5, 3: 2.5}[kind], kappa, group)
	return O.linear(a, b, kappa, offset, group)


def workspace(L, n, q, d, dtype=torch.float64):
	lib = L.load()
	return torch.empty((int(lib.stpy_gram_workspace_bytes(L.dtype_code(dtype), n, q, d)),), dtype=torch.uint8, device="cuda:0")


@pytest.mark.parametrize("use_ws", [False, True])
@pytest.mark.parametrize("name,kind", KINDS)
@pytest.mark.parametrize("n,q,d", [(5, 7, 3), (128, 64, 16), (300, 131, 1), (257, 513, 33), (256, 384, 16)])
def test_gram_kinds(L, name, kind, n, q, d, use_ws):
	"""use_ws=False: direct tile kernel; True: MFMA contraction + fused epilogue (not for Matern 1/2)"""
	ws = workspace(L, n, q, d) if use_ws else None
	WORK, WORK_BYTES = L.ptr(ws), (ws.numel() * ws.element_size() if ws is not None else 0)
	rng = np.random.RandomState(n + q + d + kind)
	a, b = rng.uniform(-1, 1, size=(n, d)), rng.uniform(-1, 1, size=(q, d))
	inv_ls = rng.uniform(0.3, 1.5, size=d) if kind != 4 else np.ones(d)
	ad, bd, ild = dev(a), dev(b), dev(inv_ls)
	out = torch.empty((q, n), dtype=torch.float64, device="cuda:0")
	lib = L.load()
	L.check(lib.stpy_gram(kind, L.F64, L.ptr(ad), n, d, L.ptr(bd), q, d, d, None, L.ptr(ild), 1.3, 0.25, 0.0, 0, 0,
						  L.ptr(out), n, WORK, WORK_BYTES, L.stream_ptr()), "gram")
	ref = oracle_gram(kind, a, b, inv_ls, 1.3, 0.25, None)
	assert out.shape == (q, n)
	assert rel_err(out.cpu().numpy(), ref) < 1e-13


@pytest.mark.parametrize("kind", [0, 2, 3, 4])
@pytest.mark.parametrize("d", [3, 16, 40])
def test_gram_dedicated_fill_kernel(L, kind, d):
	"""Aligned overwriting fp64 fills take the dedicated fill kernel (stpy_tune route key 28 = 1: 128 x 64 tiles, three workgroups per
	CU, points straight from L2 in MFMA fragment order): rectangular and lower-only square fills with the diagonal term, against the
	oracle and against the fused GEMM epilogue (key 28 = 0), to rounding; a padded output leading dimension keeps its padding."""
	lib = L.load()
	rng = np.random.RandomState(100 * kind + d)
	n, q = 384, 640
	a, b = rng.uniform(-1, 1, size=(n, d)), rng.uniform(-1, 1, size=(q, d))
	inv_ls = rng.uniform(0.3, 1.5, size=d) if kind != 4 else np.ones(d)
	ad, bd, ild = dev(a), dev(b), dev(inv_ls)
	ws = workspace(L, max(n, q), max(n, q), d)
	WB = ws.numel() * ws.element_size()
	assert lib.stpy_tune_get(28) == 1
	outs = {}
	try:
		for route in (1, 0):
			lib.stpy_tune(28, route)
			out = torch.full((q, n + 2), -7.0, dtype=torch.float64, device="cuda:0")          # leading dimension n + 2: padding must survive
			L.check(lib.stpy_gram(kind, L.F64, L.ptr(ad), n, d, L.ptr(bd), q, d, d, None, L.ptr(ild), 1.3, 0.25, 0.0, 0, 0,
								  L.ptr(out), n + 2, L.ptr(ws), WB, L.stream_ptr()), "gram")
			sq = torch.full((q, q), -7.0, dtype=torch.float64, device="cuda:0")
			L.check(lib.stpy_gram(kind, L.F64, L.ptr(bd), q, d, L.ptr(bd), q, d, d, None, L.ptr(ild), 0.8, 0.0, 0.37, 1, 0,
								  L.ptr(sq), q, L.ptr(ws), WB, L.stream_ptr()), "gram")
			outs[route] = (out.cpu().numpy(), sq.cpu().numpy())
	finally:
		lib.stpy_tune(28, 1)
	ref = oracle_gram(kind, a, b, inv_ls, 1.3, 0.25, None)
	refsq = oracle_gram(kind, b, b, inv_ls, 0.8, 0.0, None) + 0.37 * np.eye(q)
	tiles = np.arange(q)[:, None] // 128 >= np.arange(q)[None, :] // 128
	for route, (o, s2) in outs.items():
		assert rel_err(o[:, :n], ref) < 1e-13, route
		assert np.all(o[:, n:] == -7.0), route
		assert rel_err(s2[tiles], refsq[tiles]) < 1e-13, route
		assert np.all(s2[~tiles] == -7.0), route          # tiles strictly above the diagonal untouched
	assert rel_err(outs[1][0][:, :n], outs[0][0][:, :n]) < 1e-14


@pytest.mark.parametrize("use_ws", [False, True])
def test_gram_cols_combine_diag_lower(L, use_ws):
	rng = np.random.RandomState(3)
	n, d = 333, 6
	ws = workspace(L, n, n, d) if use_ws else None
	WORK, WORK_BYTES = L.ptr(ws), (ws.numel() * ws.element_size() if ws is not None else 0)
	x = rng.uniform(-1, 1, size=(n, d))
	xd = dev(x)
	cols = [0, 2, 5]
	inv_ls = np.array([1.0, 0.5, 2.0])
	colsd = torch.tensor(cols, dtype=torch.int32, device="cuda:0")
	lib = L.load()
	out = torch.empty((n, n), dtype=torch.float64, device="cuda:0")
	ild, il2d = dev(inv_ls), dev(np.full(d, 0.7))
	L.check(lib.stpy_gram(0, L.F64, L.ptr(xd), n, d, L.ptr(xd), n, d, 3, L.ptr(colsd), L.ptr(ild), 1.1, 0.0, 0.0, 0, L.OUT_SET,
						  L.ptr(out), n, WORK, WORK_BYTES, L.stream_ptr()), "gram")
	k1 = oracle_gram(0, x, x, inv_ls, 1.1, 0.0, cols)
	assert rel_err(out.cpu().numpy(), k1) < 1e-13
	# product with a Matern 5/2 on all columns, then diag_add on the last item
	il2 = np.full(d, 0.7)
	L.check(lib.stpy_gram(3, L.F64, L.ptr(xd), n, d, L.ptr(xd), n, d, d, None, L.ptr(il2d), 0.9, 0.0, 0.04, 0, L.OUT_MUL,
						  L.ptr(out), n, WORK, WORK_BYTES, L.stream_ptr()), "gram")
	k2 = k1 * oracle_gram(3, x, x, il2, 0.9, 0.0, None) + 0.04 * np.eye(n)
	assert rel_err(out.cpu().numpy(), k2) < 1e-13
	# lower_only: lower triangle identical, sum with ADD
	out2 = torch.full((n, n), 7.0, dtype=torch.float64, device="cuda:0")
	L.check(lib.stpy_gram(0, L.F64, L.ptr(xd), n, d, L.ptr(xd), n, d, 3, L.ptr(colsd), L.ptr(ild), 1.1, 0.0, 0.5, 1, L.OUT_SET,
						  L.ptr(out2), n, WORK, WORK_BYTES, L.stream_ptr()), "gram")
	o2 = out2.cpu().numpy()
	il = np.tril_indices(n)
	assert rel_err(o2[il], (k1 + 0.5 * np.eye(n))[il]) < 1e-13
	assert o2[0, n - 1] == 7.0          # far upper-right tile untouched


def test_gram_diag_and_symmetrize(L):
	rng = np.random.RandomState(4)
	m, d = 77, 5
	x = rng.uniform(-1, 1, size=(m, d))
	xd = dev(x)
	lib = L.load()
	out = torch.empty((m,), dtype=torch.float64, device="cuda:0")
	il = dev(np.full(d, 0.5))
	L.check(lib.stpy_gram_diag(0, L.F64, L.ptr(xd), m, d, d, None, L.ptr(il), 1.7, 0.0, L.OUT_SET, L.ptr(out), L.stream_ptr()), "diag")
	assert np.allclose(out.cpu().numpy(), 1.7, rtol=0, atol=0)
	ones = dev(np.ones(d))
	L.check(lib.stpy_gram_diag(4, L.F64, L.ptr(xd), m, d, d, None, L.ptr(ones), 2.0, 0.5, L.OUT_ADD, L.ptr(out), L.stream_ptr()), "diag")
	assert rel_err(out.cpu().numpy(), 1.7 + 2.0 * np.sum(x * x, axis=1) + 0.5) < 1e-14
	n = 200
	A = rng.normal(size=(n, n))
	Ad = dev(A)
	L.check(lib.stpy_symmetrize_lower(L.F64, n, L.ptr(Ad), n, L.stream_ptr()), "sym")
	ref = np.tril(A) + np.tril(A, -1).T
	assert np.array_equal(Ad.cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------ factorisation + solves
def run_potrf(L, K, nb=0, dtype=torch.float64, flags=0):
	lib = L.load()
	n = K.shape[0]
	Kd = dev(K, dtype)
	code = L.dtype_code(dtype)
	winv = torch.empty((int(lib.stpy_potrf_winv_elems(n)),), dtype=dtype, device="cuda:0")
	work = torch.empty((int(lib.stpy_potrf_workspace_bytes(code, n, nb)),), dtype=torch.uint8, device="cuda:0")
	info = torch.full((1,), -5, dtype=torch.int32, device="cuda:0")
	L.check(lib.stpy_potrf(code, n, L.ptr(Kd), n, L.ptr(winv), winv.numel(), L.ptr(work), work.numel() * work.element_size(), nb, flags, L.ptr(info), L.stream_ptr()), "potrf")
	return Kd, winv, int(info.item())


@pytest.mark.parametrize("n,nb", [(1, 0), (64, 0), (128, 0), (129, 0), (200, 128), (512, 256), (1000, 256), (1536, 512), (2049, 512), (3000, 0)])
def test_potrf(L, n, nb):
	rng = np.random.RandomState(n)
	K = spd(rng, n)
	Ld, winv, info = run_potrf(L, K, nb)
	assert info == 0
	Lg = np.tril(Ld.cpu().numpy())
	Lref = np.linalg.cholesky(K)
	assert rel_err(Lg, Lref) < 1e-12
	assert rel_err(Lg @ Lg.T, K) < 1e-14
	# cached inverse diagonal blocks
	W = winv.cpu().numpy().reshape(-1, 128, 128)
	for bi in range(W.shape[0]):
		c = bi * 128
		cb = min(128, n - c)
		Wref = np.linalg.inv(Lref[c:c + cb, c:c + cb])
		assert rel_err(W[bi][:cb, :cb], Wref) < 1e-11
		assert np.all(np.triu(W[bi], 1) == 0)


def test_f32_factor_presplit_route_is_bit_identical(L):
	"""Route key 32 (gemm_bf3p.hip): the fp32 factorisation splits each finished panel ONCE into its three bf16 planes and runs both trailing
	updates from those; with the switch off every tile of the update re-splits its operands on the fly (gemm_nt_bf3_kernel).  The arithmetic
	per output element is the same sequence of matrix-core instructions, so the two factors must agree bit for bit -- and both against fp64."""
	lib = L.load()
	n = 6144                       # panels of 512: trailing matrices of 5632 .. 2048 rows take the planes, the rest the on-the-fly kernel
	rng = np.random.RandomState(5)
	x = rng.uniform(-1, 1, size=(n, 6))
	xx = (x * x).sum(1)
	K = np.exp(-0.5 * np.maximum(xx[:, None] + xx[None, :] - 2 * x @ x.T, 0) / 0.3 ** 2) + 0.05 * np.eye(n)
	assert lib.stpy_tune_get(32) == 1
	outs = []
	keep30 = int(lib.stpy_tune_get(30))
	lib.stpy_tune(30, 0)          # (with the few-tile route on, route 0 would take its mid-size updates onto the fp32 MFMA: a different comparison)
	try:
		for route in (0, 1):
			lib.stpy_tune(32, route)
			Ld, winv, info = run_potrf(L, K, 0, torch.float32)
			assert info == 0
			outs.append((torch.tril(Ld).clone(), winv.clone()))
	finally:
		lib.stpy_tune(32, 1)
		lib.stpy_tune(30, keep30)
	assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
	Lref = np.linalg.cholesky(K)
	assert rel_err(outs[1][0].cpu().numpy().astype(np.float64), Lref) < 2e-5
	# the workspace query covers the planes: two fp32 panel buffers + three bf16 planes of one panel
	nb = 512
	assert int(lib.stpy_potrf_workspace_bytes(L.F32, n, nb)) == 2 * n * nb * 4 + 3 * n * nb * 2
	assert int(lib.stpy_potrf_workspace_bytes(L.F64, n, nb)) == 2 * n * nb * 8


def test_potrf_not_positive_definite(L):
	rng = np.random.RandomState(0)
	n = 300
	K = spd(rng, n)
	K[170, 170] = -1.0
	_, _, info = run_potrf(L, K, 128)
	assert info == 171          # LAPACK convention: order of the failing leading minor


@pytest.mark.parametrize("n,m,nb", [(128, 5, 0), (200, 130, 128), (1000, 77, 256), (1536, 256, 512), (2049, 300, 512), (6400, 200, 1024), (5000, 129, 0)])
def test_trsm_trsv_predict_logdet(L, n, m, nb):
	rng = np.random.RandomState(n + m)
	K = spd(rng, n)
	Ld, winv, info = run_potrf(L, K, nb)
	assert info == 0
	Lref = np.linalg.cholesky(K)
	lib = L.load()
	B = rng.normal(size=(m, n))
	Bd = dev(B)
	L.check(lib.stpy_trsm_right_lt(L.F64, m, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(Bd), n, nb, 0, None, 0, L.stream_ptr()), "trsm")
	Xref = sla.solve_triangular(Lref, B.T, lower=True).T
	assert rel_err(Bd.cpu().numpy(), Xref) < 1e-11
	# the same solve with the K-pass workspace
	# (below n = 32768 the library keeps the right-looking sweep; stpy_tune(5, 2) forces the left-looking form)
	assert int(lib.stpy_trsm_workspace_bytes(L.F64, m, n, nb)) == 0
	lib.stpy_tune(5, 2)
	try:
		wb = int(lib.stpy_trsm_workspace_bytes(L.F64, m, n, nb))
		assert (wb == 0) == (n <= (nb if nb > 0 else 512))
		Bw = dev(B)
		wk = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda:0")
		L.check(lib.stpy_trsm_right_lt(L.F64, m, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(Bw), n, nb, 0, L.ptr(wk), wk.numel() * wk.element_size(), L.stream_ptr()), "trsm")
		assert rel_err(Bw.cpu().numpy(), Xref) < 1e-11
		# right-looking sweep and the recursive form (the default from 2048 rows on) with 128-, 256- and 512-column leaves
		for alg in (1, 3, 4, 5):
			lib.stpy_tune(5, alg)
			assert alg == 1 or int(lib.stpy_trsm_workspace_bytes(L.F64, m, n, nb)) == 0
			Ba = dev(B)
			L.check(lib.stpy_trsm_right_lt(L.F64, m, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(Ba), n, nb, 0, None, 0, L.stream_ptr()), "trsm")
			assert rel_err(Ba.cpu().numpy(), Xref) < 1e-11, alg
	finally:
		lib.stpy_tune(5, 0)
	y = rng.normal(size=n)
	yd, zd, ad = dev(y), torch.empty(n, dtype=torch.float64, device="cuda:0"), torch.empty(n, dtype=torch.float64, device="cuda:0")
	L.check(lib.stpy_trsv(L.F64, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(yd), L.ptr(zd), 0, L.stream_ptr()), "trsv")
	zref = sla.solve_triangular(Lref, y, lower=True)
	assert rel_err(zd.cpu().numpy(), zref) < 1e-11
	zs = zd.clone()
	L.check(lib.stpy_trsv(L.F64, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(zs), L.ptr(ad), 1, L.stream_ptr()), "trsv")
	aref = sla.solve_triangular(Lref.T, zref, lower=False)
	assert rel_err(ad.cpu().numpy(), aref) < 1e-10
	kdiag = np.full(m, 5.0 + np.max(np.sum(Xref * Xref, axis=1)))
	mu, sg = torch.empty(m, dtype=torch.float64, device="cuda:0"), torch.empty(m, dtype=torch.float64, device="cuda:0")
	kdd = dev(kdiag)
	L.check(lib.stpy_predict(L.F64, m, n, L.ptr(Bd), n, L.ptr(zd), L.ptr(kdd), L.ptr(mu), L.ptr(sg), 0, L.stream_ptr()), "predict")
	assert rel_err(mu.cpu().numpy(), Xref @ zref) < 1e-11
	assert rel_err(sg.cpu().numpy(), np.sqrt(kdiag - np.sum(Xref * Xref, axis=1))) < 1e-12
	out2 = torch.empty(2, dtype=torch.float64, device="cuda:0")
	L.check(lib.stpy_logdet_quad(L.F64, n, L.ptr(Ld), n, L.ptr(zd), L.ptr(out2), L.stream_ptr()), "logdet")
	o = out2.cpu().numpy()
	assert abs(o[0] - np.sum(np.log(np.diag(Lref)))) < 1e-10 * max(1.0, abs(o[0]))
	assert abs(o[1] - zref @ zref) < 1e-10 * abs(zref @ zref)


@pytest.mark.parametrize("n,nb", [(128, 0), (300, 128), (1024, 256), (1500, 0)])
def test_potri(L, n, nb):
	"""K^-1 from the factor: upper-triangular-aware trsm + K-skipping SYRK"""
	rng = np.random.RandomState(n + 1)
	K = spd(rng, n)
	Ld, winv, info = run_potrf(L, K, nb)
	assert info == 0
	lib = L.load()
	Kinv = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda:0")
	work = torch.empty((n, n), dtype=torch.float64, device="cuda:0")
	L.check(lib.stpy_potri(L.F64, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(Kinv), n, L.ptr(work), work.numel() * work.element_size(), L.stream_ptr()), "potri")
	out = Kinv.cpu().numpy()
	ref = np.linalg.inv(K)
	il = np.tril_indices(n)
	assert rel_err(out[il], ref[il]) < 1e-10
	# the scratch buffer holds L^-T (upper triangular)
	LinvT = np.linalg.inv(np.linalg.cholesky(K)).T
	assert rel_err(np.triu(work.cpu().numpy()), LinvT) < 1e-10


def test_predict_negative_variance_is_nan_unless_clamped(L):
	"""gauss_procc.py:394-395: sqrt of an unclamped difference."""
	lib = L.load()
	X = dev(np.array([[2.0, 0.0], [0.5, 0.5]]))
	z = dev(np.array([1.0, 1.0]))
	kd = dev(np.array([1.0, 1.0]))
	mu, sg = torch.empty(2, dtype=torch.float64, device="cuda:0"), torch.empty(2, dtype=torch.float64, device="cuda:0")
	L.check(lib.stpy_predict(L.F64, 2, 2, L.ptr(X), 2, L.ptr(z), L.ptr(kd), L.ptr(mu), L.ptr(sg), 0, L.stream_ptr()), "predict")
	s = sg.cpu().numpy()
	assert np.isnan(s[0]) and abs(s[1] - np.sqrt(0.5)) < 1e-15
	L.check(lib.stpy_predict(L.F64, 2, 2, L.ptr(X), 2, L.ptr(z), L.ptr(kd), L.ptr(mu), L.ptr(sg), 1, L.stream_ptr()), "predict")
	assert sg.cpu().numpy()[0] == 0.0


def test_potrf_f32(L):
	rng = np.random.RandomState(11)
	n = 1000
	K = spd(rng, n, s=0.5)
	Ld, winv, info = run_potrf(L, K.astype(np.float32), 256, torch.float32)
	assert info == 0
	Lg = np.tril(Ld.cpu().numpy().astype(np.float64))
	assert rel_err(Lg @ Lg.T, K) < 5e-6


# ------------------------------------------------------------------------------------------ RFF
@pytest.mark.parametrize("n,d,m", [(33, 5, 64), (200, 64, 130), (129, 1, 256)])
def test_rff(L, n, d, m):
	rng = np.random.RandomState(n + d + m)
	x, W, b = rng.uniform(0, 1, size=(n, d)), rng.normal(size=(m, d)) / 0.7, 2 * np.pi * rng.uniform(size=m)
	lib = L.load()
	out = torch.empty((n, m), dtype=torch.float64, device="cuda:0")
	scale = np.sqrt(2.0 / m) * np.sqrt(2.5)
	xd, Wd, bd = dev(x), dev(W), dev(b)          # keep the device buffers alive across the launches
	L.check(lib.stpy_rff_embed(L.F64, L.ptr(xd), n, d, d, L.ptr(Wd), d, m, None, None, scale, L.ptr(out), m, 0, None, 0, L.stream_ptr()), "rff")
	assert rel_err(out.cpu().numpy(), O.rff_embed(x, W, m, kappa=2.5)) < 1e-14
	L.check(lib.stpy_rff_embed(L.F64, L.ptr(xd), n, d, d, L.ptr(Wd), d, m, L.ptr(bd), None, scale, L.ptr(out), m, 0, None, 0, L.stream_ptr()), "rff")
	assert rel_err(out.cpu().numpy(), O.rff_embed(x, W, m, kappa=2.5, b=b).T) < 1e-14


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-14), (torch.float32, 2e-5)])
def test_rff_transposed(L, dtype, tol):
	rng = np.random.RandomState(21)
	n, d, m = 300, 7, 130
	x, W, b = rng.uniform(0, 1, size=(n, d)), rng.normal(size=(m, d)) / 0.7, 2 * np.pi * rng.uniform(size=m)
	lib = L.load()
	xd, Wd, bd = dev(x, dtype), dev(W, dtype), dev(b, dtype)
	out = torch.empty((m, n), dtype=dtype, device="cuda:0")
	scale = np.sqrt(2.0 / m)
	L.check(lib.stpy_rff_embed(L.dtype_code(dtype), L.ptr(xd), n, d, d, L.ptr(Wd), d, m, None, None, scale, L.ptr(out), n, 1, None, 0, L.stream_ptr()), "rff")
	ref = O.rff_embed(x, W, m).T
	assert np.abs(out.cpu().numpy() - ref).max() < tol * 10 * np.abs(ref).max() + tol * 1e-2
	L.check(lib.stpy_rff_embed(L.dtype_code(dtype), L.ptr(xd), n, d, d, L.ptr(Wd), d, m, L.ptr(bd), None, scale, L.ptr(out), n, 1, None, 0, L.stream_ptr()), "rff")
	ref = O.rff_embed(x, W, m, b=b)          # the reference's biased orientation is already (m, n)
	assert np.abs(out.cpu().numpy() - ref).max() < tol * 10 * np.abs(ref).max() + tol * 1e-2


def test_trsm_many_rows_default_is_recursive(L):
	"""m >= 2048 rows: the default block solve is the recursive form (no workspace), ragged n included"""
	lib = L.load()
	for n, m in ((1000, 2048), (1536, 2100)):
		rng = np.random.RandomState(n + m)
		K = spd(rng, n)
		Ld, winv, info = run_potrf(L, K, 0)
		assert info == 0
		assert int(lib.stpy_trsm_workspace_bytes(L.F64, m, n, 0)) == 0
		B = rng.normal(size=(m, n))
		Bd = dev(B)
		L.check(lib.stpy_trsm_right_lt(L.F64, m, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(Bd), n, 0, 0, None, 0, L.stream_ptr()), "trsm")
		Xref = sla.solve_triangular(np.linalg.cholesky(K), B.T, lower=True).T
		assert rel_err(Bd.cpu().numpy(), Xref) < 1e-11


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-11), (torch.float32, 2e-4)])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_potrf_panel_strip_modes(L, mode, dtype, tol):
	"""stpy_tune key 18: how the rows below a panel's diagonal block are solved -- two products per 128 columns beside the update (0),
	one strip launch on the look-ahead stream (1; 2: first panel only), or one strip launch on the update's stream after the
	trailing update (3).  Same factor and inverse blocks in every mode; aligned and ragged orders, a failing pivot reported alike."""
	lib = L.load()
	if mode != 0 and lib.stpy_tune_get(18) < 0:
		pytest.skip("strip modes 1-3 are measured-and-dropped experiments: lab build only (STPY_HIP_LIB=lab)")
	lib.stpy_tune(18, mode)
	try:
		for n, nb in ((2048 + 256, 512), (1500, 256), (4096, 0)):
			rng = np.random.RandomState(n + 3)
			K = spd(rng, n)
			Ld, winv, info = run_potrf(L, K, nb, dtype)
			assert info == 0
			Lref = np.linalg.cholesky(K)
			assert rel_err(np.tril(Ld.cpu().numpy().astype(np.float64)), Lref) < tol
			W = winv.cpu().numpy().astype(np.float64).reshape(-1, 128, 128)
			for bi in (0, (n + 127) // 128 - 1):
				c, cb = bi * 128, min(128, n - bi * 128)
				assert rel_err(W[bi][:cb, :cb], np.linalg.inv(Lref[c:c + cb, c:c + cb])) < tol * 100
		K = spd(np.random.RandomState(9), 1536)
		K[1100, 1100] = -1.0
		_, _, info = run_potrf(L, K, 256, dtype)
		assert info == 1101
	finally:
		lib.stpy_tune(18, 0)


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-11), (torch.float32, 3e-4)])
@pytest.mark.parametrize("strip", [512, 1024, 0, 1])
def test_trsm_strip_leaf(L, strip, dtype, tol):
	"""recursive block solve with its leaves (up to 512 / 1024 columns) as one strip launch each (stpy_tune key 17; 0 = the
	three-launch leaves): same X as scipy for n a power of two, n with a ragged tail, row counts that are / are not multiples of
	the strip's 16 rows (the kernel guards the rest), a single row; fp64 and fp32"""
	lib = L.load()
	lib.stpy_tune(17, strip)
	lib.stpy_tune(5, 4)          # recursive form whatever the row count
	code = L.dtype_code(dtype)
	try:
		for n, m in ((2048, 2048), (1536 + 70, 144), (1024, 16), (640, 100), (384, 1), (896, 333)):
			rng = np.random.RandomState(n + m + 1)
			K = spd(rng, n)
			Ld, winv, info = run_potrf(L, K, 0, dtype)
			assert info == 0
			B = rng.normal(size=(m, n))
			Bd = dev(B, dtype)
			L.check(lib.stpy_trsm_right_lt(code, m, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(Bd), n, 0, 0, None, 0, L.stream_ptr()), "trsm")
			Xref = sla.solve_triangular(np.linalg.cholesky(K), B.T, lower=True).T
			assert rel_err(Bd.cpu().numpy().astype(np.float64), Xref) < tol, (n, m)
	finally:
		lib.stpy_tune(17, 1)
		lib.stpy_tune(5, 0)


@pytest.mark.parametrize("n,d,m", [(300, 64, 512), (256, 64, 512), (384, 32, 256), (128, 96, 128), (128, 64, 192), (640, 32, 64)])
def test_rff_f32(L, n, d, m):
	"""fp32 embed: the dedicated 128 x 64 tile kernel (d = 32 / 64, n % 128 == 0, m % 64 == 0; m = 192 puts the cos / sin
	boundary inside a tile) and the trig fused into the GEMM's store for every other shape (ragged: register staging;
	d = 96 and the transposed outputs: LDS-DMA, K tiles of 32 floats); plain / biased / transposed"""
	rng = np.random.RandomState(2 + n + d + m)
	x, W = rng.uniform(0, 1, size=(n, d)).astype(np.float32), (rng.normal(size=(m, d)) / 8.0).astype(np.float32)
	b = (2 * np.pi * rng.uniform(size=m)).astype(np.float32)
	lib = L.load()
	xd, Wd, bd = dev(x, torch.float32), dev(W, torch.float32), dev(b, torch.float32)
	x64, W64, b64 = x.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
	scale = float(np.sqrt(2.0 / m))
	out = torch.empty((n, m), dtype=torch.float32, device="cuda:0")
	L.check(lib.stpy_rff_embed(L.F32, L.ptr(xd), n, d, d, L.ptr(Wd), d, m, None, None, scale, L.ptr(out), m, 0, None, 0, L.stream_ptr()), "rff")
	ref = O.rff_embed(x64, W64, m)
	assert np.abs(out.cpu().numpy() - ref).max() < 2e-5 * np.abs(ref).max()
	L.check(lib.stpy_rff_embed(L.F32, L.ptr(xd), n, d, d, L.ptr(Wd), d, m, L.ptr(bd), None, scale, L.ptr(out), m, 0, None, 0, L.stream_ptr()), "rff")
	refb = O.rff_embed(x64, W64, m, b=b64)            # (m, n) in the reference's biased orientation
	assert np.abs(out.cpu().numpy() - refb.T).max() < 2e-5 * np.abs(refb).max()
	outT = torch.empty((m, n), dtype=torch.float32, device="cuda:0")
	L.check(lib.stpy_rff_embed(L.F32, L.ptr(xd), n, d, d, L.ptr(Wd), d, m, None, None, scale, L.ptr(outT), n, 1, None, 0, L.stream_ptr()), "rff")
	assert np.abs(outT.cpu().numpy() - ref.T).max() < 2e-5 * np.abs(ref).max()
	L.check(lib.stpy_rff_embed(L.F32, L.ptr(xd), n, d, d, L.ptr(Wd), d, m, L.ptr(bd), None, scale, L.ptr(outT), n, 1, None, 0, L.stream_ptr()), "rff")
	assert np.abs(outT.cpu().numpy() - refb).max() < 2e-5 * np.abs(refb).max()


def test_rff_f32_tile_kernel_matches_gemm_epilogue(L):
	"""the two fp32 routes (stpy_tune key 9) on one tile-aligned problem, with a padded output leading dimension"""
	n, d, m, ldo = 512, 64, 320, 384
	rng = np.random.RandomState(11)
	x, W = rng.uniform(-3, 3, size=(n, d)).astype(np.float32), (rng.normal(size=(m, d)) / 4.0).astype(np.float32)
	b = (2 * np.pi * rng.uniform(size=m)).astype(np.float32)
	lib = L.load()
	xd, Wd, bd = dev(x, torch.float32), dev(W, torch.float32), dev(b, torch.float32)
	scale = float(np.sqrt(2.0 / m))
	outs = {}
	assert lib.stpy_tune_get(9) == 1
	try:
		for route in (1, 0):
			lib.stpy_tune(9, route)
			for bias in (None, bd):
				out = torch.full((n, ldo), 7.0, dtype=torch.float32, device="cuda:0")
				L.check(lib.stpy_rff_embed(L.F32, L.ptr(xd), n, d, d, L.ptr(Wd), d, m, L.ptr(bias) if bias is not None else None, None, scale, L.ptr(out), ldo, 0, None, 0, L.stream_ptr()), "rff")
				outs[(route, bias is not None)] = out.cpu().numpy()
	finally:
		lib.stpy_tune(9, 1)
	for biased in (False, True):
		a, g = outs[(1, biased)], outs[(0, biased)]
		assert np.all(a[:, m:] == 7.0) and np.all(g[:, m:] == 7.0)          # nothing written beyond column m
		assert np.abs(a[:, :m] - g[:, :m]).max() < 1e-5 * np.abs(g[:, :m]).max()
	ref = O.rff_embed(x.astype(np.float64), W.astype(np.float64), m)
	assert np.abs(outs[(1, False)][:, :m] - ref).max() < 2e-5 * np.abs(ref).max()


def test_rff_f32_bf16_split_kernel(L):
	"""Large fp32 d = 64 shapes WITH the workspace: the contraction runs on the bf16 matrix cores from an exact three-way split
	of both operands.  Same result as the fp32-MFMA kernel to fp32 rounding level and as the oracle within the fp32 tolerance --
	on well-scaled inputs and on inputs that stress the split: mixed signs, 1e-6 .. 1e3 dynamic range inside a row, exact zeros,
	phases of tens of revolutions; plain and biased; a row count that leaves the last stride of row blocks partly idle."""
	lib = L.load()
	n, d, m = 8192 + 3 * 128, 64, 2048
	wb = int(lib.stpy_rff_workspace_bytes(L.F32, n, d, m))
	assert wb == m * 64 * 6
	assert int(lib.stpy_rff_workspace_bytes(L.F32, n, 32, m)) == 0 and int(lib.stpy_rff_workspace_bytes(L.F64, n, d, m)) == 0
	assert int(lib.stpy_rff_workspace_bytes(L.F32, 4096, d, m)) == 0 and int(lib.stpy_rff_workspace_bytes(L.F32, n, d, m + 64)) == 0
	work = torch.empty(wb, dtype=torch.uint8, device="cuda:0")
	rng = np.random.RandomState(7)
	scale = float(np.sqrt(2.0 / m))
	cases = {}
	cases["well scaled"] = (rng.uniform(-2, 2, size=(n, d)), rng.normal(size=(m, d)) / 4.0)
	xs = rng.uniform(-1, 1, size=(n, d)) * 10.0 ** rng.uniform(-6, 1, size=(n, d))
	xs[rng.uniform(size=(n, d)) < 0.1] = 0.0
	ws = rng.normal(size=(m, d)) * 10.0 ** rng.uniform(-3, 0.5, size=(m, d))
	cases["wide range, zeros"] = (xs, ws)
	cases["many revolutions"] = (rng.uniform(-8, 8, size=(n, d)), rng.normal(size=(m, d)) * 2.0)
	b = (2 * np.pi * rng.uniform(size=m)).astype(np.float32)
	bd = dev(b, torch.float32)
	for name, (x, W) in cases.items():
		x, W = x.astype(np.float32), W.astype(np.float32)
		xd, Wd = dev(x, torch.float32), dev(W, torch.float32)
		phase = np.abs(x[:256].astype(np.float64) @ W.astype(np.float64).T).max()
		# fp32 arithmetic resolves a phase of p radians to about p * 2^-23 (inputs) + the accumulation of 64 products
		tol = max(2e-5, 6e-6 * phase)
		for bias, bnp in ((None, None), (bd, b)):
			got = {}
			for use_ws in (True, False):
				out = torch.full((n, m), 7.0, dtype=torch.float32, device="cuda:0")
				L.check(lib.stpy_rff_embed(L.F32, L.ptr(xd), n, d, d, L.ptr(Wd), d, m, L.ptr(bias) if bias is not None else None, None, scale, L.ptr(out), m, 0,
										   L.ptr(work) if use_ws else None, wb if use_ws else 0, L.stream_ptr()), "rff")
				got[use_ws] = out.cpu().numpy()
			assert np.abs(got[True]).max() <= scale * (1 + 1e-6), name          # every element written (the fill value was 7)
			rows = np.r_[0:128, n - 128:n]
			ref = O.rff_embed(x[rows].astype(np.float64), W.astype(np.float64), m, b=None if bnp is None else bnp.astype(np.float64))
			ref = ref.T if bnp is not None else ref
			e_split = np.abs(got[True][rows] - ref).max() / scale
			e_f32 = np.abs(got[False][rows] - ref).max() / scale
			assert e_split < tol, (name, e_split, tol)
			assert e_split < 3 * e_f32 + 2e-6, (name, e_split, e_f32)          # as accurate as the fp32-MFMA kernel
			assert np.abs(got[True] - got[False]).max() / scale < 2 * tol, name
	# an undersized workspace is refused, not overrun
	out = torch.empty((n, m), dtype=torch.float32, device="cuda:0")
	xd, Wd = dev(cases["well scaled"][0].astype(np.float32), torch.float32), dev(cases["well scaled"][1].astype(np.float32), torch.float32)
	rc = lib.stpy_rff_embed(L.F32, L.ptr(xd), n, d, d, L.ptr(Wd), d, m, None, None, scale, L.ptr(out), m, 0, L.ptr(work), wb - 16, L.stream_ptr())
	assert rc == -20 and b"workspace" in lib.stpy_last_error_string()


def test_rff_f32_bf16_split_kernel_strided(L):
	"""the same kernel with leading dimensions larger than the logical widths (x: d + 8, W: d + 4, out: m + 64): nothing is
	written beyond column m, nothing is read beyond column d"""
	lib = L.load()
	n, d, m = 8192, 64, 1024
	rng = np.random.RandomState(11)
	xp = rng.uniform(-1, 1, size=(n, d + 8)).astype(np.float32)
	Wp = (rng.normal(size=(m, d + 4)) / 3.0).astype(np.float32)
	xp[:, d:] = 1e30          # poison: must never be read
	Wp[:, d:] = 1e30
	xd, Wd = dev(xp, torch.float32), dev(Wp, torch.float32)
	wb = int(lib.stpy_rff_workspace_bytes(L.F32, n, d, m))
	assert wb > 0
	work = torch.empty(wb, dtype=torch.uint8, device="cuda:0")
	out = torch.full((n, m + 64), 7.0, dtype=torch.float32, device="cuda:0")
	scale = float(np.sqrt(2.0 / m))
	L.check(lib.stpy_rff_embed(L.F32, L.ptr(xd), n, d + 8, d, L.ptr(Wd), d + 4, m, None, None, scale, L.ptr(out), m + 64, 0, L.ptr(work), wb, L.stream_ptr()), "rff")
	got = out.cpu().numpy()
	assert np.all(got[:, m:] == 7.0)
	ref = O.rff_embed(xp[:256, :d].astype(np.float64), Wp[:, :d].astype(np.float64), m)
	assert np.abs(got[:256, :m] - ref).max() < 2e-5 * scale
	assert np.abs(got[:, :m]).max() <= scale * (1 + 1e-6)


def test_rff_f32_bf16_split_kernel_rotated_sweep(L):
	"""every row block starts its sweep over the column part at tile 2 rb mod tiles and wraps around: a tile count per part that is
	not a power of two (m = 3072: six tiles), more row blocks than tiles, every element written exactly once and right"""
	lib = L.load()
	n, d, m = 8192 + 5 * 128, 64, 3072
	rng = np.random.RandomState(23)
	x = rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
	W = (rng.normal(size=(m, d)) / 3.0).astype(np.float32)
	xd, Wd = dev(x, torch.float32), dev(W, torch.float32)
	wb = int(lib.stpy_rff_workspace_bytes(L.F32, n, d, m))
	assert wb > 0
	work = torch.empty(wb, dtype=torch.uint8, device="cuda:0")
	out = torch.full((n, m), 7.0, dtype=torch.float32, device="cuda:0")
	scale = float(np.sqrt(2.0 / m))
	L.check(lib.stpy_rff_embed(L.F32, L.ptr(xd), n, d, d, L.ptr(Wd), d, m, None, None, scale, L.ptr(out), m, 0, L.ptr(work), wb, L.stream_ptr()), "rff")
	got = out.cpu().numpy()
	assert np.abs(got).max() <= scale * (1 + 1e-6)          # the fill value is gone everywhere
	rows = np.r_[0:128, 128 * 3:128 * 4, 128 * 37:128 * 38, n - 128:n]          # row blocks 0, 3, 37 and the last: four different rotations
	ref = O.rff_embed(x[rows].astype(np.float64), W.astype(np.float64), m)
	assert np.abs(got[rows] - ref).max() < 2e-5 * scale


def test_rff_f32_streaming_kernel(L):
	"""n >= 8192, m % 1024 == 0, d = 64: the persistent streaming kernel (stpy_tune key 9 = 1) against the tile kernel (2) and
	the GEMM epilogue (0), plain and biased, with a row count that leaves the last stride of row blocks partly idle"""
	n, d, m = 8192 + 3 * 128, 64, 2048
	rng = np.random.RandomState(5)
	x, W = rng.uniform(-2, 2, size=(n, d)).astype(np.float32), (rng.normal(size=(m, d)) / 4.0).astype(np.float32)
	b = (2 * np.pi * rng.uniform(size=m)).astype(np.float32)
	lib = L.load()
	xd, Wd, bd = dev(x, torch.float32), dev(W, torch.float32), dev(b, torch.float32)
	scale = float(np.sqrt(2.0 / m))
	outs = {}
	try:
		for route in (1, 2, 0):
			lib.stpy_tune(9, route)
			for bias in (None, bd):
				out = torch.full((n, m), 7.0, dtype=torch.float32, device="cuda:0")
				L.check(lib.stpy_rff_embed(L.F32, L.ptr(xd), n, d, d, L.ptr(Wd), d, m, L.ptr(bias) if bias is not None else None, None, scale, L.ptr(out), m, 0, None, 0, L.stream_ptr()), "rff")
				outs[(route, bias is not None)] = out.cpu().numpy()
	finally:
		lib.stpy_tune(9, 1)
	ref = O.rff_embed(x[:512].astype(np.float64), W.astype(np.float64), m)
	refb = O.rff_embed(x[:512].astype(np.float64), W.astype(np.float64), m, b=b.astype(np.float64)).T
	for biased, r in ((False, ref), (True, refb)):
		a = outs[(1, biased)]
		assert np.abs(a).max() <= scale * (1 + 1e-6)                  # every element written (the fill value was 7)
		for other in (2, 0):
			assert np.abs(a - outs[(other, biased)]).max() < 1e-5 * scale
		assert np.abs(a[:512] - r).max() < 2e-5 * np.abs(r).max()


def test_error_reporting(L):
	lib = L.load()
	WORK = None
	rc = lib.stpy_gram(99, L.F64, None, 1, 1, None, 1, 1, 1, None, None, 1.0, 0.0, 0.0, 0, 0, None, 1, WORK, 0, L.stream_ptr())
	assert rc < 0 and b"null" in lib.stpy_last_error_string()
	x = dev(np.zeros((2, 2)))
	rc = lib.stpy_gemm_nt(7, 2, 2, 2, L.ptr(x), 2, L.ptr(x), 2, L.ptr(x), 2, 0, 0, L.stream_ptr())
	assert rc < 0 and b"dtype" in lib.stpy_last_error_string()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("m,n,ldo,lds", [(300, 300, 300, 300), (257, 130, 136, 132), (5, 3, 7, 3), (1, 1000, 1000, 1000)])
def test_combine_and_predict_finish(L, dtype, m, n, ldo, lds):
	"""stpy_combine: out (set | + | *)= src on a strided window, then + diag_add on the diagonal; stpy_predict_finish:
	mu *= scale, sigma = sqrt(kdiag - scale * sumsq) (the post-all-reduce epilogue of the sharded prediction)."""
	lib = L.load()
	rng = np.random.RandomState(m + n)
	code = L.dtype_code(dtype)
	npdt = np.float64 if dtype == torch.float64 else np.float32
	for comb in (L.OUT_SET, L.OUT_ADD, L.OUT_MUL):
		a, b = rng.normal(size=(m, ldo)).astype(npdt), rng.normal(size=(m, lds)).astype(npdt)
		ad, bd = dev(a, dtype), dev(b, dtype)
		L.check(lib.stpy_combine(code, m, n, L.ptr(ad), ldo, L.ptr(bd), lds, comb, 0.25, L.stream_ptr()), "combine")
		ref = a.copy()
		w = ref[:, :n]
		w[...] = b[:, :n] if comb == L.OUT_SET else (w + b[:, :n] if comb == L.OUT_ADD else w * b[:, :n])
		k = min(m, n)
		w[np.arange(k), np.arange(k)] += npdt(0.25)
		assert np.array_equal(ad.cpu().numpy(), ref)          # elementwise: exact, and nothing outside the window is touched
	assert lib.stpy_combine(code, m, n, L.ptr(ad), n - 1, L.ptr(bd), lds, 0, 0.0, L.stream_ptr()) == -5
	mu, ss, kd = rng.normal(size=m).astype(npdt), rng.uniform(0, 1, size=m).astype(npdt), rng.uniform(1, 2, size=m).astype(npdt)
	mud, ssd, kdd = dev(mu, dtype), dev(ss, dtype), dev(kd, dtype)
	sg = torch.empty(m, dtype=dtype, device="cuda:0")
	L.check(lib.stpy_predict_finish(code, m, L.ptr(mud), L.ptr(ssd), L.ptr(kdd), 0.5, L.ptr(sg), 0, L.stream_ptr()), "predict_finish")
	tol = 1e-15 if dtype == torch.float64 else 1e-6
	assert rel_err(mud.cpu().numpy(), mu * npdt(0.5)) < tol and rel_err(sg.cpu().numpy(), np.sqrt(kd - npdt(0.5) * ss)) < tol


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-4)])
@pytest.mark.parametrize("n,nb", [(128, 0), (1024, 256), (2048, 512), (3200, 1024), (1000, 256), (4096, 0)])
def test_potrf_and_trsm_beside_update(L, dtype, tol, n, nb):
	"""STPY_FLAG_BESIDE_UPDATE routes every block of the call through the kernels that fit into what two trailing-update
	workgroups leave over on a CU: the 32 x 128 "sliver" GEMM (fp64; other shapes fall back to the tile kernels).  Same factor, same inverse blocks, same solve as without the flag; the failing
	pivot is reported at the same index."""
	lib = L.load()
	rng = np.random.RandomState(n + 5)
	K = spd(rng, n)
	Ld, winv, info = run_potrf(L, K, nb, dtype, flags=L.FLAG_BESIDE_UPDATE)
	Ld0, winv0, info0 = run_potrf(L, K, nb, dtype, flags=0)
	assert info == 0 and info0 == 0
	Lg = np.tril(Ld.cpu().numpy().astype(np.float64))
	Lref = np.linalg.cholesky(K)
	assert rel_err(Lg, Lref) < tol
	assert rel_err(Lg, np.tril(Ld0.cpu().numpy().astype(np.float64))) < tol
	W = winv.cpu().numpy().astype(np.float64).reshape(-1, 128, 128)
	for bi in range((n + 127) // 128):
		c, cb = bi * 128, min(128, n - bi * 128)
		assert rel_err(W[bi][:cb, :cb], np.linalg.inv(Lref[c:c + cb, c:c + cb])) < tol * 100
		assert np.all(np.triu(W[bi], 1) == 0)
	m = 320
	B = rng.normal(size=(m, n))
	Bd = dev(B, dtype)
	code = L.dtype_code(dtype)
	L.check(lib.stpy_trsm_right_lt(code, m, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(Bd), n, nb, L.FLAG_BESIDE_UPDATE, None, 0, L.stream_ptr()), "trsm")
	Xref = sla.solve_triangular(Lref, B.T, lower=True).T
	assert rel_err(Bd.cpu().numpy().astype(np.float64), Xref) < tol * 10
	if n >= 1024:          # a matrix that stops being positive definite at a known pivot
		Kb = K.copy()
		Kb[700, 700] = -1.0
		_, _, infob = run_potrf(L, Kb, nb, dtype, flags=L.FLAG_BESIDE_UPDATE)
		assert infob == 701


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-11), (torch.float32, 3e-4)])
@pytest.mark.parametrize("n", [512, 1024, 4096, 8192 + 128])
def test_trsv_one_launch_dataflow(L, dtype, tol, n):
	"""n a multiple of 128 (>= 512): both vector solves run as ONE launch each -- a dataflow over the 128-blocks with
	write-through hand-off of the solved blocks (stpy_tune key 16 = 1, the default) -- and agree with scipy and, to rounding,
	with the chain of per-block launches (key 16 = 0); repeated calls reuse the 64-byte sync area correctly."""
	lib = L.load()
	rng = np.random.RandomState(n)
	K = spd(rng, n)
	Ld, winv, info = run_potrf(L, K, 0, dtype)
	assert info == 0
	Lref = np.linalg.cholesky(K)
	code = L.dtype_code(dtype)
	y = rng.normal(size=n)
	zref = sla.solve_triangular(Lref, y, lower=True)
	aref = sla.solve_triangular(Lref.T, zref, lower=False)
	outs = {}
	try:
		for mode in (1, 0, 1):
			lib.stpy_tune(16, mode)
			yd = dev(y, dtype)
			zd, ad = torch.full((n,), float("nan"), dtype=dtype, device="cuda:0"), torch.full((n,), float("nan"), dtype=dtype, device="cuda:0")
			L.check(lib.stpy_trsv(code, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(yd), L.ptr(zd), 0, L.stream_ptr()), "trsv")
			zs = zd.clone()
			L.check(lib.stpy_trsv(code, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(zs), L.ptr(ad), 1, L.stream_ptr()), "trsv")
			outs[mode] = (zd.cpu().numpy().astype(np.float64), ad.cpu().numpy().astype(np.float64))
			assert rel_err(outs[mode][0], zref) < tol and rel_err(outs[mode][1], aref) < tol * 10
	finally:
		lib.stpy_tune(16, 1)
	assert rel_err(outs[1][0], outs[0][0]) < tol and rel_err(outs[1][1], outs[0][1]) < tol * 10
	assert lib.stpy_async_status(L.stream_ptr()) == 0


def test_trsv_handoff_timeout_is_loud(L):
	"""A hand-off wait of the one-launch vector solve that gives up must not return silently wrong numbers: the output is NaN
	from the affected block on and stpy_async_status reports (and clears) the sticky device error word.  The fault is injected
	with the lab build's test hook (stpy_tune key 22: the block with that ticket is never published); the product library has
	no such hook, there the test only checks that a clean solve reports status 0."""
	lib = L.load()
	n = 2048
	rng = np.random.RandomState(5)
	K = spd(rng, n)
	Ld, winv, info = run_potrf(L, K, 0, torch.float64)
	y = rng.normal(size=n)
	if lib.stpy_tune_get(22) == -1:
		yd, zd = dev(y), torch.empty(n, dtype=torch.float64, device="cuda:0")
		L.check(lib.stpy_trsv(L.F64, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(yd), L.ptr(zd), 0, L.stream_ptr()), "trsv")
		assert lib.stpy_async_status(L.stream_ptr()) == 0 and not torch.isnan(zd).any()
		pytest.skip("fault injection needs the lab build (STPY_HIP_LIB=lab)")
	lib.stpy_tune(22, 3 + 1)          # ticket 3 is never published
	try:
		yd, zd = dev(y), torch.zeros(n, dtype=torch.float64, device="cuda:0")
		L.check(lib.stpy_trsv(L.F64, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(yd), L.ptr(zd), 0, L.stream_ptr()), "trsv")
		assert lib.stpy_async_status(L.stream_ptr()) == 1
		z = zd.cpu().numpy()
		assert not np.isnan(z[:4 * 128]).any() and np.isnan(z[4 * 128:]).all()          # blocks 0..3 solved, block 4 timed out, the rest inherit
		assert lib.stpy_async_status(L.stream_ptr()) == 0                               # read-and-clear
	finally:
		lib.stpy_tune(22, 0)
	yd, zd = dev(y), torch.empty(n, dtype=torch.float64, device="cuda:0")
	L.check(lib.stpy_trsv(L.F64, n, L.ptr(Ld), n, L.ptr(winv), winv.numel(), L.ptr(yd), L.ptr(zd), 0, L.stream_ptr()), "trsv")
	assert lib.stpy_async_status(L.stream_ptr()) == 0
	assert rel_err(zd.cpu().numpy(), sla.solve_triangular(np.linalg.cholesky(K), y, lower=True)) < 1e-11


# ------------------------------------------------------------------------------------------ small reductions / layout helpers (reduce.hip)
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-14), (torch.float32, 1e-6)])
@pytest.mark.parametrize("n", [1, 63, 64, 130, 1000])
def test_tril_trace_dot(L, dtype, tol, n):
	lib = L.load()
	rng = np.random.RandomState(n)
	code = L.dtype_code(dtype)
	ld = n + 3
	A = rng.normal(size=(n, ld))
	Ad = dev(A, dtype)
	u, v = rng.normal(size=n), rng.normal(size=n)
	ud, vd = dev(u, dtype), dev(v, dtype)
	out = torch.full((2,), float("nan"), dtype=dtype, device="cuda:0")
	L.check(lib.stpy_trace_dot(code, n, L.ptr(Ad), ld, L.ptr(ud), L.ptr(vd), L.ptr(out), L.stream_ptr()), "trace_dot")
	o = out.cpu().numpy().astype(np.float64)
	scale = np.abs(np.diag(A[:, :n])).sum() + 1
	assert abs(o[0] - np.trace(A[:, :n])) / scale < tol * 10 and abs(o[1] - u @ v) / (np.abs(u * v).sum() + 1) < tol * 10
	L.check(lib.stpy_trace_dot(code, n, None, 0, None, None, L.ptr(out), L.stream_ptr()), "trace_dot")
	assert out.cpu().tolist() == [0.0, 0.0]
	L.check(lib.stpy_tril(code, n, L.ptr(Ad), ld, L.stream_ptr()), "tril")
	got = Ad.cpu().numpy().astype(np.float64)
	ref = A.astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64)
	ref[:, :n] = np.tril(ref[:, :n])
	assert np.array_equal(got, ref)          # (the padding columns beyond n are untouched)
	assert lib.stpy_tril(code, n, L.ptr(Ad), n - 1, L.stream_ptr()) == -4 if n > 1 else True


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-4)])
def test_scaled_points_and_lml_grad_reduce(L, dtype, tol):
	"""stpy_scaled_points_t builds [Xs | 1]^T; stpy_lml_grad_reduce turns P = H [Xs | 1] into the per-parameter sums
	inv_ls_k/2 sum_ij H_ij (xs_ik - xs_jk)^2 accumulated at acc[pidx[k]] (checked against that double sum directly)."""
	lib = L.load()
	rng = np.random.RandomState(3)
	code = L.dtype_code(dtype)
	n, dfull = 700, 6
	cols = [4, 0, 2]
	inv = np.array([0.7, 1.9, 0.4])
	x = rng.uniform(-1, 1, size=(n, dfull))
	xd = dev(x, dtype)
	for use_cols in (True, False):
		c = cols if use_cols else [0, 1, 2]
		d = len(c)
		cd = torch.tensor(c, dtype=torch.int32, device="cuda:0") if use_cols else None
		invd = dev(inv, dtype)
		XT = torch.full((d + 1, n + 5), float("nan"), dtype=dtype, device="cuda:0")
		L.check(lib.stpy_scaled_points_t(code, L.ptr(xd), n, dfull, d, L.ptr(cd), L.ptr(invd), L.ptr(XT), n + 5, 1, L.stream_ptr()), "scaled_points_t")
		xs = x[:, c] * inv
		got = XT.cpu().numpy().astype(np.float64)
		assert rel_err(got[:d, :n], xs.T) < (1e-15 if dtype == torch.float64 else 1e-7) and np.all(got[d, :n] == 1.0) and np.isnan(got[:, n:]).all()
		H = rng.normal(size=(n, n)); H = H + H.T
		P = H @ np.concatenate([xs, np.ones((n, 1))], axis=1)
		pidx = [1, 0, 1]
		acc0 = np.array([0.25, -1.5])
		acc = dev(acc0, dtype)
		Pd, pd = dev(P, dtype), torch.tensor(pidx, dtype=torch.int32, device="cuda:0")
		L.check(lib.stpy_lml_grad_reduce(code, L.ptr(xd), n, dfull, d, L.ptr(cd), L.ptr(invd), L.ptr(Pd), d + 1, L.ptr(pd), L.ptr(acc), L.stream_ptr()), "lml_grad_reduce")
		ref = acc0.copy()
		for k in range(d):
			diff = xs[:, k:k + 1] - xs[:, k:k + 1].T
			ref[pidx[k]] += inv[k] * 0.5 * np.sum(H * diff * diff)
		scale = np.abs(H).sum()
		assert np.max(np.abs(acc.cpu().numpy().astype(np.float64) - ref)) / scale < tol


def test_async_status_raises_through_the_classes(L, monkeypatch):
	"""A non-zero stpy_async_status (a hand-off wait of the one-launch vector solve that gave up: NaN results) must surface as an
	exception from GaussianProcess.fit_gp and KernelizedFeatures.fit_gp, and leave the object unfitted.  The product library has no
	fault hook, so the status word is stubbed on the host side; the device-side fault itself is covered by
	test_trsv_handoff_timeout_is_loud on the lab build."""
	import stpy_amd
	from stpy_amd.continuous_processes.kernelized_features import KernelizedFeatures
	lib = L.load()
	rng = np.random.RandomState(0)
	x = torch.from_numpy(rng.uniform(-1, 1, size=(300, 2)))
	y = torch.from_numpy(np.sin(x.numpy().sum(axis=1, keepdims=True)))
	GP = stpy_amd.GaussianProcess(gamma=0.5, s=0.1, kernel_name="squared_exponential", d=2)
	GP.fit_gp(x, y)
	assert GP.fitted
	monkeypatch.setattr(lib, "stpy_async_status", lambda stream: 1)
	with pytest.raises(L.StpyHipError, match="stpy_async_status"):
		GP.fit_gp(x, y)
	assert GP.fitted is False
	emb = stpy_amd.RFFEmbedding(gamma=0.5, m=32, d=2)
	KF = KernelizedFeatures(embedding=emb, m=32, s=0.1, d=2)
	with pytest.raises(L.StpyHipError, match="stpy_async_status"):
		KF.fit_gp(x, y)
	assert KF.fitted is False
	monkeypatch.undo()
	KF.fit_gp(x, y)
	GP.fit_gp(x, y)
	assert KF.fitted and GP.fitted


@pytest.mark.timeout(900)
def test_lab_only_cases_in_a_child_interpreter():
	"""The fault-injection test of the one-launch vector solve and the measured-and-dropped strip modes need the LAB build of the library
	(experiment hooks the product library does not carry), so in a plain `pytest -m gpu` run they skip.  This runs exactly those cases in
	a child interpreter with STPY_HIP_LIB=lab, so that the suite's record covers them: none of them may fail OR skip there."""
	import os
	import subprocess
	import sys
	root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
	if os.environ.get("STPY_HIP_LIB", "") == "lab":
		pytest.skip("already the lab run")
	if not os.path.exists(os.path.join(root, "stpy_amd", "libstpy_hip_lab.so")):
		pytest.skip("no lab build in this tree (make -C stpy_amd/csrc EXPERIMENTS=1)")
	env = dict(os.environ, STPY_HIP_LIB="lab")
	# exactly the options below (none added through the environment), in an interpreter set up like this one: a suite run that
	# ignores the user's site-packages (python -s) must not load pytest plugins from there in the child
	env.pop("PYTEST_ADDOPTS", None)
	py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
	r = subprocess.run(py + ["-m", "pytest", os.path.join(root, "tests", "test_gpu_kernels.py"), "-q", "-m", "gpu", "-x", "-rs", "-p", "no:cacheprovider",
						"-k", "test_trsv_handoff_timeout_is_loud or test_potrf_panel_strip_modes"], capture_output=True, text=True, timeout=800, cwd=root, env=env)
	tail = r.stdout[-3000:] + r.stderr[-2000:]
	assert r.returncode == 0, tail
	assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], tail
