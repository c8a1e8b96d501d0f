"""
stpy_gemm_nt_bc (the trailing update of the distributed Cholesky) through the C ABI, in GLOBAL coordinates: one process plays every
rank of a process grid in turn, the local results are gathered, and the expectation is "the lower 128-tile triangle of the global
matrix" from tests/bc_cases.py -- an oracle that enumerates the distribution and does not know the kernel's index formula.

Every comparison is entry by entry against an fp64 torch.matmul reference:

    |got - ref| <= f * gamma_{S (k+1)} * (|C0| + sum_K |P_K| |P_K|^T),   gamma_n = n u / (1 - n u)

S updates applied (1 for single calls; the sweeps use the largest count, nblk - 1, for every entry), u = 2^-53 (fp64) or 2^-24 (fp32),
f = 2 for fp64 (the reference carries the same error) and 1 for fp32.  This is the standard bound of an inner product accumulated by
fused multiply-adds in any order, which both MFMA types are.  A skipped, doubled or mis-addressed tile is off by the bracket itself.
Run with `-m gpu -s` to see the worst error / bound of every case.
"""
import time

import pytest
import torch

from tests import bc_cases as bc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def L(gpu_device):
	from stpy_amd import _lib
	return _lib


def gen(seed):
	return torch.Generator(device=DEV).manual_seed(seed)


def randn(g, *shape, dtype=F64):
	return torch.randn(*shape, dtype=dtype, device=DEV, generator=g)


def raw_call(L, dtype, m, n, k, A, lda, B, ldb, C, ldc, mode, w):
	return int(L.load().stpy_gemm_nt_bc(L.dtype_code(dtype), m, n, k, L.ptr(A), lda, L.ptr(B), ldb, L.ptr(C), ldc, mode, *[int(v) for v in w], L.stream_ptr()))


def call(L, A, B, C, mode, w):
	"""return code of stpy_gemm_nt_bc on tensors / strided views"""
	return raw_call(L, C.dtype, A.shape[0], B.shape[0], A.shape[1], A, L.ld(A), B, L.ld(B), C, L.ld(C), mode, w)


def last_error(L):
	return L.load().stpy_last_error_string().decode("utf-8", "replace")


# ------------------------------------------------------------------------------------------ (a) whole sweeps
@pytest.mark.parametrize("pr,pc,N,NB,k,dtype", [
	(1, 1, 1280, 256, 128, F64),         # baseline: the staircase of one rank is the global lower triangle
	(1, 2, 2500, 256, 128, F64),         # ragged last block: guarded kernel on the ranks that hold it, direct-to-VGPR kernel on the others
	(1, 2, 2500, 256, 128, F32),
	(2, 2, 6144, 128, 128, F64),         # local 3072 x 3072: 3 x 3 super-tiles, the staircase passes through every one over 47 steps
	(2, 4, 4296, 256, 128, F64),         # the default grid of 8 ranks, ragged
	(2, 4, 4296, 256, 128, F32),
	(4, 2, 3072, 128, 64, F64),          # more process rows than columns
	(4, 2, 3072, 128, 64, F32),          # (fp32 at k = 64: the aligned LDS tile kernel, not direct-to-VGPR)
	(2, 4, 8192, 2048, 32, F64),         # the 8-GPU configuration's block: diagonal blocks of 16 x 16 tiles, lower ones only; k = 32: aligned non-dtv kernel
], ids=lambda v: {F64: "f64", F32: "f32"}.get(v, str(v)))
def test_sweep_gathers_to_the_global_lower_tile_update(L, pr, pc, N, NB, k, dtype):
	g = gen(N + NB + 16 * pr + pc + k)
	nblk = (N + NB - 1) // NB
	C0 = randn(g, N, N, dtype=dtype)
	panels = [randn(g, N, k, dtype=dtype) for _ in range(nblk - 1)]

	def one(A, B, C, w):
		L.check(call(L, A, B, C, 1, w), "gemm_nt_bc %s" % (w,))

	got = bc.sweep(one, C0, panels, NB, pr, pc, "split")
	single = bc.sweep(one, C0, panels, NB, pr, pc, "single")
	again = bc.sweep(one, C0, panels, NB, pr, pc, "split")
	torch.cuda.synchronize()
	ref, bracket, low = bc.sweep_reference(C0, panels, NB)
	ratio = bc.worst_ratio(got, ref, bracket, nblk - 1, k, dtype)
	print("\nsweep %dx%d N=%d NB=%d k=%d %s: worst error / bound %.3g" % (pr, pc, N, NB, k, str(dtype)[6:], ratio))
	assert torch.equal(got[~low], C0[~low])                 # every tile strictly above the global tile diagonal keeps its bits
	assert ratio <= 1.0
	assert torch.equal(single, got)                         # one call per step or the look-ahead's two: same bits
	assert torch.equal(again, got)                          # and the same bits on every run


# ------------------------------------------------------------------------------------------ (b) single calls on one window
M, N_, K_ = 1152, 896, 128
CROSS = (256, 2, 4, 0, 2, 1, 0)            # rows: global blocks 2, 4, 6, 8, 10 (the last one half); columns: 2, 6, 10, 14 (half) -- three diagonal blocks
ABOVE = (256, 2, 4, 0, 3, 0, 2)            # rows 0 .. 8, columns 11, 15, ..: wholly above the staircase
BELOW = (256, 2, 4, 1, 0, 10, 0)           # rows 21 .., columns 0 .. 12: wholly below
LDC, OFF = 1032, 72                        # the window sits inside a wider buffer


def window_case(L, dtype, mode, w, poison):
	"""one call on the M x N_ window of a NaN-filled buffer.  poison: the tiles the oracle marks as not needed are NaN as well (and in
	mode 0 the needed ones too: they are overwritten, never read).  Returns (rc, buf, win, C0, need, want, bracket)."""
	g = gen(1000 * mode + sum(w) + (dtype == F32))
	A, B, C0 = randn(g, M, K_, dtype=dtype), randn(g, N_, K_, dtype=dtype), randn(g, M, N_, dtype=dtype)
	need = bc.expand_tiles(bc.needed_mask(M, N_, *w), M, N_, DEV)
	buf = torch.full((M, LDC), NAN, dtype=dtype, device=DEV)
	win = buf[:, OFF:OFF + N_]
	if not poison:
		win.copy_(C0)
	elif mode != 0:
		win.copy_(torch.where(need, C0, torch.full_like(C0, NAN)))
	rc = call(L, A, B, win, mode, w)
	torch.cuda.synchronize()
	prod = A.double() @ B.double().T
	want = {0: prod, 1: C0.double() - prod, 2: C0.double() + prod}[mode]
	bracket = A.double().abs() @ B.double().abs().T + (C0.double().abs() if mode != 0 else 0.0)
	return rc, buf, win, C0, need, want, bracket


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_window_crossing_the_staircase(L, dtype, mode):
	rc, buf, win, C0, need, want, bracket = window_case(L, dtype, mode, CROSS, poison=True)
	assert rc == 0, last_error(L)
	assert bool(need.any()) and not bool(need.all())
	assert bool(torch.isfinite(win[need]).all())                             # every needed tile written ...
	ratio = bc.worst_ratio(win[need], want[need], bracket[need], 1, K_, dtype)
	print("\nwindow crossing, mode %d %s: worst error / bound %.3g" % (mode, str(dtype)[6:], ratio))
	assert ratio <= 1.0                                                      # ... and correct
	assert bool(torch.isnan(win[~need]).all())                               # the others neither read into a result nor written
	assert bool(torch.isnan(buf[:, :OFF]).all()) and bool(torch.isnan(buf[:, OFF + N_:]).all())
	# (NaN -= x stays NaN: that the other tiles are not WRITTEN in modes 1 and 2 shows on finite data, as the same bits)
	rc, buf, win2, C0, need, want, bracket = window_case(L, dtype, mode, CROSS, poison=False)
	assert rc == 0, last_error(L)
	assert torch.equal(win2[~need], C0[~need])
	assert torch.equal(win2[need], win[need])


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_window_above_the_staircase_is_left_alone(L, dtype):
	for mode in (0, 1, 2):
		rc, buf, win, C0, need, want, bracket = window_case(L, dtype, mode, ABOVE, poison=False)
		assert rc == 0, last_error(L)
		assert not bool(need.any())
		assert torch.equal(win, C0), mode
		assert bool(torch.isnan(buf[:, :OFF]).all()) and bool(torch.isnan(buf[:, OFF + N_:]).all())


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_window_below_the_staircase_is_the_plain_product(L, dtype):
	for mode in (0, 1, 2):
		rc, buf, win, C0, need, want, bracket = window_case(L, dtype, mode, BELOW, poison=True)
		assert rc == 0, last_error(L)
		assert bool(need.all())
		ratio = bc.worst_ratio(win, want, bracket, 1, K_, dtype)
		print("\nwindow below, mode %d %s: worst error / bound %.3g" % (mode, str(dtype)[6:], ratio))
		assert ratio <= 1.0, mode
		assert bool(torch.isnan(buf[:, :OFF]).all()) and bool(torch.isnan(buf[:, OFF + N_:]).all())


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_return_codes(L, dtype):
	"""the argument checks of stpy_gemm_nt_bc as include/stpy_hip.h states them; every refusal returns before any launch"""
	g = gen(77)
	m, n, k = 256, 256, 128
	A, B, C0 = randn(g, m, k, dtype=dtype), randn(g, n, k, dtype=dtype), randn(g, m, n, dtype=dtype)
	C = C0.clone()
	ok = (128, 1, 1, 0, 0, 0, 0)

	def rc_of(mode, w, kk=k):
		return raw_call(L, dtype, m, n, kk, A, k, B, k, C, n, mode, w)

	for mode in (-1, 3, 4, 5, 6, 7):                       # 3, 4 and 5 are internal numbers of the GEMM: not reachable from outside
		assert rc_of(mode, ok) == -11, mode
		msg = last_error(L)
		assert all(s in msg for s in ("C = A B^T", "C -= A B^T", "C += A B^T")), msg
	for nbd in (0, -128, 100, 127, 192):
		assert rc_of(1, (nbd,) + ok[1:]) == -13, nbd
	for w in ((128, 0, 1, 0, 0, 0, 0), (128, 1, 0, 0, 0, 0, 0), (128, 2, 2, -1, 0, 0, 0), (128, 2, 2, 2, 0, 0, 0), (128, 2, 2, 0, -1, 0, 0),
	          (128, 2, 2, 0, 2, 0, 0), (128, 2, 2, 0, 0, -1, 0), (128, 2, 2, 0, 0, 0, -1)):
		assert rc_of(1, w) == -13, w
	assert rc_of(1, ok, 0) == 0 and rc_of(2, ok, 0) == 0           # k = 0: nothing to subtract / add
	assert rc_of(0, ok, 0) == -4                                   # ... and the overwrite form keeps its refusal
	torch.cuda.synchronize()
	assert torch.equal(C, C0)                                      # none of the above touched C
	assert rc_of(2, ok) == 0, last_error(L)                        # mode 2 is C += A B^T, as in stpy_gemm_nt
	torch.cuda.synchronize()
	low = bc.lower_tiles(m, DEV)
	want = C0.double() + torch.where(low, A.double() @ B.double().T, torch.zeros((), dtype=F64, device=DEV))
	assert bc.worst_ratio(C, want, C0.double().abs() + A.double().abs() @ B.double().abs().T, 1, k, dtype) <= 1.0


# ------------------------------------------------------------------------------------------ (c) the prefix-table limit
LIMIT = (1024, 1, 30, 0, 4, 0, 0)          # column blocks: global 4, 34, 64; row blocks: 0, 1, 2, ...


@pytest.mark.parametrize("m,embedded", [
	(65536, False),          # 64 super-tile rows: the last size the host's prefix table holds (compact enumeration)
	(66560, False),          # 65 rows: rotated rectangle; the only case in which column block 64 receives work
	(65496, False),          # the same two, ragged: the guarded kernel's copy of the enumeration
	(66520, False),
	(65536, True),           # C = the last 3072 columns of a 65 536 x 32 768 buffer: the last tile rows lie beyond 2^32 bytes from the window's base
])
def test_prefix_table_limit(L, m, embedded):
	"""fp64, mode 1, k = 128, n = 3072 (8 x 8-tile super-tiles, the shortest there are), distribution block 1024 on a 1 x 30 grid: the table has
	empty leading rows (row blocks 0 .. 3), diagonal blocks at I = 4 and I = 34, and a third column only row block 64 needs"""
	n, k = 3072, 128
	t_start = time.perf_counter()
	mask = bc.needed_mask(m, n, *LIMIT)
	assert not bool(mask[:32].any()) and bool(mask[32, 0]) and not bool(mask[32, 1])          # the shape described above, from the oracle
	assert bool(mask[:, 16:].any()) == (m > 65536)
	g = gen(m + embedded)
	A, B = randn(g, m, k), randn(g, n, k)
	buf = None
	try:
		if embedded:
			buf = torch.empty((m, 32768), dtype=F64, device=DEV)          # uninitialised: only the window is filled
			C = buf[:, 32768 - n:]
			C.copy_(randn(g, m, n))
		else:
			C = randn(g, m, n)
		C0 = C.clone()
		torch.cuda.synchronize()
		t_call = time.perf_counter()
		rc = call(L, A, B, C, 1, LIMIT)
		torch.cuda.synchronize()
		t_call = time.perf_counter() - t_call
		assert rc == 0, last_error(L)
		need = bc.expand_tiles(mask, m, n, DEV)
		assert bool(((C == C0) | need).all())                             # tiles above the staircase keep their bits
		prod = A @ B.T
		ref = torch.where(need, C0 - prod, C0)
		del prod
		bracket = A.abs() @ B.abs().T
		bracket += C0.abs()
		ratio = bc.worst_ratio(C, ref, bracket, 1, k, F64)
		print("\nlimit m=%d%s: worst error / bound %.3g, call %.3f s, test %.2f s" % (m, " (embedded)" if embedded else "", ratio, t_call, time.perf_counter() - t_start))
		assert ratio <= 1.0
	finally:
		del buf
		C = C0 = ref = bracket = need = None
		torch.cuda.empty_cache()          # (gigabytes: not left with the caching allocator for the rest of the suite)
