"""
Row deletion from the resident Cholesky factor (stpy_potrf_delete / GaussianProcess.remove_data_point), the parts that need no GPU:
the interface is declared everywhere it has to be, the workspace query, every refusal of the C entry point (all of them come before
the first HIP call, so placeholder pointers are safe), the index normaliser, and a NumPy statement of the identity the device code
implements -- the compacted triangle L[R,R] updated by the rotations of cholupdate.hip with U = L[R,S] is chol(K[R,R] + s^2 I).  The
NumPy form is also what tests/test_gpu_gp_remove.py explains its expectations with.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT, rel_err

IB = 128
CU_KC = 32          # columns of U per rotation pass (cholupdate.hip)


def pad(n):
	return -(-int(n) // IB) * IB


# --------------------------------------------------------------------------------------------- 1. the interface exists
def test_header_declares_delete():
	with open(os.path.join(ROOT, "include", "stpy_hip.h")) as f:
		h = f.read()
	assert "int64_t stpy_potrf_delete_workspace_bytes(int dtype, int64_t n0, int64_t k);" in h
	assert "int stpy_potrf_delete(int dtype, int64_t n0, int64_t k, const int32_t* del_host," in h
	assert "HOST pointer" in h          # the one host pointer of the ABI is announced as such


def test_signatures_list_delete():
	from stpy_amd import _lib
	assert _lib.SIGNATURES["stpy_potrf_delete_workspace_bytes"] == (_lib._i64, [_lib._i32, _lib._i64, _lib._i64])
	res, args = _lib.SIGNATURES["stpy_potrf_delete"]
	assert res is _lib._i32 and len(args) == 14
	assert callable(_lib.potrf_delete)


# --------------------------------------------------------------------------------------------- 2. workspace query
def test_workspace_query():
	from stpy_amd import _lib as L
	lib = L.load()
	q = lib.stpy_potrf_delete_workspace_bytes
	for dt in (0, 1):
		assert q(dt, 300, 0) == 0 and q(dt, 300, -1) == 0 and q(dt, 0, 0) == 0
		last = 0
		for n0 in (2, 127, 128, 129, 300, 1030, 4096, 16384, 65536):
			b = q(dt, n0, 1)
			assert b > 0 and b % 16 == 0 and b >= last, (dt, n0, b, last)
			last = b
		last = 0
		for k in (1, 2, 3, 8, 31, 32, 33, 40, 127, 128, 129, 500, 1029):
			b = q(dt, 1030, k)
			assert b > 0 and b % 16 == 0 and b >= last, (dt, k, b, last)
			last = b
		# it holds what the header says it holds: the indices, the index map and U
		assert q(dt, 1030, 40) >= 40 * 4 + pad(1030 - 40) * 4 + pad(1030 - 40) * 40 * (8 if dt == 0 else 4)


# --------------------------------------------------------------------------------------------- 3. argument checks
def test_potrf_delete_argument_checks():
	from stpy_amd import _lib as L
	lib = L.load()
	N = None
	PA, PB, P = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x40000000), ctypes.c_void_p(0x1000)      # never dereferenced by a refused call
	big = 1 << 40

	def ids(*v):
		return (ctypes.c_int32 * len(v))(*v)

	def call(dtype=0, n0=300, k=3, idx=ids(5, 17, 299), A=PA, lda=384, B=PB, ldb=384, winv=P, winv_elems=big, work=P, work_bytes=big, info=P):
		return lib.stpy_potrf_delete(dtype, n0, k, idx, A, lda, B, ldb, winv, winv_elems, work, work_bytes, info, N)

	esz = 8
	refused = {
		"unknown dtype": (dict(dtype=7), -1),
		"n0 = 0": (dict(n0=0, k=-1), -2), "n0 < 0": (dict(n0=-5), -2),
		"k < 0": (dict(k=-1), -3), "k = n0": (dict(n0=3), -3), "k > n0": (dict(n0=2), -3),
		"null del_host": (dict(idx=N), -4), "null A": (dict(A=N), -5), "null B": (dict(B=N), -7), "null winv": (dict(winv=N), -9),
		"null work": (dict(work=N), -11), "null info_dev": (dict(info=N), -13),
		"unsorted": (dict(idx=ids(17, 5, 299)), -15), "duplicate": (dict(idx=ids(5, 5, 299)), -15),
		"index = n0": (dict(idx=ids(5, 17, 300)), -15), "negative index": (dict(idx=ids(-1, 17, 299)), -15),
		"lda < pad(n0)": (dict(lda=383), -6), "ldb < pad(n1)": (dict(n0=385, idx=ids(127, 128, 129), lda=512, ldb=383), -8),
		"B inside A": (dict(B=ctypes.c_void_p(0x10000000 + 384 * 100 * esz)), -16), "B = A": (dict(B=PA), -16),
		"A inside B": (dict(A=ctypes.c_void_p(0x40000000 + 8)), -16),
		"B ends inside A": (dict(B=ctypes.c_void_p(0x10000000 - 16)), -16),
		"winv too small": (dict(winv_elems=3 * IB * IB - 1), -21),
		"workspace too small": (dict(work_bytes=lib.stpy_potrf_delete_workspace_bytes(0, 300, 3) - 1), -20),
		"fp32 workspace too small": (dict(dtype=1, work_bytes=lib.stpy_potrf_delete_workspace_bytes(1, 300, 3) - 1), -20),
	}
	kind_of = {}
	for what, (kw, code) in refused.items():
		lib.stpy_chol_update(7, 256, 2, 1, P, 256, P, 1 << 20, P, 2, P, 1 << 30, P, N)          # (leaves some OTHER message behind)
		before = lib.stpy_last_error_string()
		rc = call(**kw)
		assert rc == code, (what, rc)
		msg = lib.stpy_last_error_string()
		assert msg and b"stpy_potrf_delete" in msg and msg != before, (what, msg)
		kind_of.setdefault(code, set()).add(what)
	# each kind of refusal has a code of its own: the fifteen of the header
	assert sorted(kind_of) == [-21, -20, -16, -15, -13, -11, -9, -8, -7, -6, -5, -4, -3, -2, -1], kind_of
	# nothing to delete: 0 without looking at a pointer
	assert lib.stpy_potrf_delete(0, 300, 0, N, N, 0, N, 0, N, 0, N, 0, N, N) == 0
	# and a request every check passes would go on to the device: not tried here


# --------------------------------------------------------------------------------------------- 4. index normaliser
def test_normalize_remove_index():
	from stpy_amd.continuous_processes.gauss_procc import normalize_remove_index as f
	assert f(3, 10) == [3] and f(-1, 10) == [9] and f(np.int64(4), 10) == [4]
	assert f([7, 2, 5], 10) == [2, 5, 7] and f((0, -10 + 9), 10) == [0, 9] and f(range(2, 5), 10) == [2, 3, 4]
	assert f(torch.tensor([4, -2, 0]), 10) == [0, 4, 8] and f(torch.tensor(6), 10) == [6] and f(np.array([1, 0], dtype=np.int32), 10) == [0, 1]
	assert f([], 10) == [] and f(torch.zeros((0,), dtype=torch.long), 10) == []
	for bad in ([1, 1], [1, -9], torch.tensor([0, 0]), (3, 5, 3)):
		with pytest.raises(ValueError):
			f(bad, 10)
	for bad in (10, -11, [0, 10], torch.tensor([5, -11])):
		with pytest.raises(IndexError):
			f(bad, 10)
	with pytest.raises(ValueError):
		f(torch.zeros((2, 2), dtype=torch.long), 10)
	for bad in (1.5, [0.0], torch.tensor([1.0]), "3", True, torch.tensor([True])):
		with pytest.raises(TypeError):
			f(bad, 10)


def test_remove_needs_fitted_data_without_a_gpu():
	"""the refusals that come before any device work"""
	from stpy_amd import GaussianProcess
	GP = GaussianProcess(gamma=0.5, s=0.3, d=3)
	assert GP.remove_path is None and GP.delete_max_rank == 128 and GaussianProcess.remove_data is GaussianProcess.remove_data_point
	for it in (False, True):
		with pytest.raises(ValueError):
			GP.remove_data_point(0, iterative=it)
	assert GP.x is None and GP.n == 0 and GP.fitted is False and GP._factor is None


# --------------------------------------------------------------------------------------------- 5. the identity, in NumPy
def se_gram(x, gamma=0.5, kappa=1.0, s=0.3):
	d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
	return kappa * np.exp(-0.5 * d2 / gamma ** 2) + s ** 2 * np.eye(x.shape[0])


_rng = np.random.RandomState(11)          # the recipe of tests/test_gp_append.py: the same first rows of the same stream
X_ALL = _rng.uniform(0, 1, size=(4096 + 300, 3))[:1100]


def kept(n0, S):
	gone = set(S)
	return [i for i in range(n0) if i not in gone]


def deleted_factor_numpy(L, S, dtype=np.float64):
	"""What stpy_potrf_delete computes, restated: B = L[R,R], U = L[R,S] (zero on and right of the diagonal), then the rotation
	recurrence of cholupdate.hip with sign = +1, chunks of 32 columns of U, from the block column of S[0].  Returns (B, first block
	column visited or None when U is zero)."""
	n0 = L.shape[0]
	R = kept(n0, S)
	L = np.tril(L).astype(dtype)
	B = L[np.ix_(R, R)].copy()
	U = L[np.ix_(R, S)].copy()
	U[np.asarray(R)[:, None] <= np.asarray(S)[None, :]] = 0
	n1 = len(R)
	if S[0] >= n1:
		assert not U.any()
		return B, None
	c_start = (S[0] // IB) * IB
	assert not U[:S[0]].any()
	for k0 in range(0, len(S), CU_KC):
		W = U[:, k0:k0 + CU_KC]
		for j in range(c_start, n1):
			d = B[j, j] * B[j, j]
			lcol = B[j + 1:, j]
			for r in range(W.shape[1]):
				wr = W[j, r]
				d1 = d + wr * wr
				a, b = np.sqrt(d), np.sqrt(d1)
				cs, sn, ic = b / a, wr / a, a / b
				lcol = (lcol + sn * W[j + 1:, r]) * ic
				W[j + 1:, r] = cs * W[j + 1:, r] - sn * lcol
				d = d1
			B[j + 1:, j] = lcol
			B[j, j] = np.sqrt(d)
			W[j] = 0
	return B, c_start


CASES = [(300, [0]), (385, [127, 128, 129]), (640, list(range(100, 140)))]


@pytest.mark.parametrize("n0,S", CASES, ids=["300-first", "385-straddle", "640-k40"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_identity_in_numpy(n0, S, dtype):
	K = se_gram(X_ALL[:n0])
	R = kept(n0, S)
	L = np.linalg.cholesky(K)
	B, c_start = deleted_factor_numpy(L.astype(dtype), S, dtype)
	ref = np.linalg.cholesky(K[np.ix_(R, R)])
	err = rel_err(B, ref)
	print("n0 %d k %d %s: factor against the refit %.2e" % (n0, len(S), np.dtype(dtype).name, err))
	assert B.dtype == dtype and c_start == (S[0] // IB) * IB
	assert err < (1e-11 if dtype == np.float64 else 1e-4)          # the bounds the GPU test uses for the same comparison
	assert np.array_equal(B[:, :c_start], L.astype(dtype)[np.ix_(R, R)][:, :c_start])          # the block columns on the left are copies
	# deleting the last rows needs no rotation at all
	B2, c2 = deleted_factor_numpy(L.astype(dtype), [n0 - 2, n0 - 1], dtype)
	assert c2 is None and np.array_equal(B2, np.tril(L.astype(dtype))[:n0 - 2, :n0 - 2])
