"""
ctypes binding of libstpy_hip.so (include/stpy_hip.h), and the typed wrappers through which the rest of the package launches:
this is the one module that knows the calling convention (dtype codes, leading dimensions, workspace / winv sizing, the
status word, the stream).

The shared library is built in-tree by ``__graft_entry__.build()`` / ``make -C stpy_amd/csrc``.
There is no CPU fallback: if the library is missing, or no ROCm device is visible, the product
path raises -- a silently different code path would void every parity claim.
PyTorch is used for device memory, streams and (multi-GPU) torch.distributed only.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# STPY_HIP_LIB=lab selects the lab build (make -C stpy_amd/csrc EXPERIMENTS=1: the product kernels plus the experiment knobs and the
# measured-and-dropped variants tools/ compares against); unset = the product library.  Same C ABI either way.
LIB_PATH = os.path.join(_HERE, "libstpy_hip_lab.so" if os.environ.get("STPY_HIP_LIB", "") == "lab" else "libstpy_hip.so")

F64, F32 = 0, 1
K_SE, K_MATERN12, K_MATERN32, K_MATERN52, K_LINEAR, K_POLY = 0, 1, 2, 3, 4, 5
OUT_SET, OUT_ADD, OUT_MUL = 0, 1, 2
IB = 128
FLAG_BESIDE_UPDATE = 1

_c = ctypes
_vp, _i64, _i32, _dbl = _c.c_void_p, _c.c_int64, _c.c_int, _c.c_double

# name -> (restype, argtypes); mirrors include/stpy_hip.h one to one
SIGNATURES = {
	"stpy_version": (_c.c_char_p, []),
	"stpy_last_error_string": (_c.c_char_p, []),
	"stpy_gram": (_i32, [_i32, _i32, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _dbl, _dbl, _i32, _i32, _vp, _i64, _vp, _i64, _vp]),
	"stpy_gram_workspace_bytes": (_i64, [_i32, _i64, _i64, _i32]),
	"stpy_gram_diag": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _dbl, _i32, _vp, _vp]),
	"stpy_potrf_workspace_bytes": (_i64, [_i32, _i64, _i32]),
	"stpy_potrf_winv_elems": (_i64, [_i64]),
	"stpy_potrf": (_i32, [_i32, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp]),
	"stpy_potrf_append_workspace_bytes": (_i64, [_i32, _i64, _i64]),
	"stpy_potrf_append": (_i32, [_i32, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp]),
	"stpy_chol_update_workspace_bytes": (_i64, [_i32, _i64, _i64]),
	"stpy_chol_update": (_i32, [_i32, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
	"stpy_potrf_delete_workspace_bytes": (_i64, [_i32, _i64, _i64]),
	"stpy_potrf_delete": (_i32, [_i32, _i64, _i64, _c.POINTER(_c.c_int32), _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
	"stpy_trsm_workspace_bytes": (_i64, [_i32, _i64, _i64, _i32]),
	"stpy_trsm_right_lt": (_i32, [_i32, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _i64, _vp]),
	"stpy_potri": (_i32, [_i32, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
	"stpy_lml_weight": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _dbl, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
	"stpy_predict_finish": (_i32, [_i32, _i64, _vp, _vp, _vp, _dbl, _vp, _i32, _vp]),
	"stpy_combine": (_i32, [_i32, _i64, _i64, _vp, _i64, _vp, _i64, _i32, _dbl, _vp]),
	"stpy_trsv": (_i32, [_i32, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp]),
	"stpy_predict": (_i32, [_i32, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _vp]),
	"stpy_logdet_quad": (_i32, [_i32, _i64, _vp, _i64, _vp, _vp, _vp]),
	"stpy_gemm_nt": (_i32, [_i32, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp]),
	"stpy_syrk_workspace_bytes": (_i64, [_i32, _i64, _i64]),
	"stpy_syrk": (_i32, [_i32, _i64, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp]),
	"stpy_gemm_nt_splitk_passes": (_i32, [_i64, _i64, _i64]),
	"stpy_gemm_nt_splitk": (_i32, [_i32, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _i64, _vp]),
	"stpy_gemm_nt_bc": (_i32, [_i32, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
	"stpy_symmetrize_lower": (_i32, [_i32, _i64, _vp, _i64, _vp]),
	"stpy_tril": (_i32, [_i32, _i64, _vp, _i64, _vp]),
	"stpy_trace_dot": (_i32, [_i32, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
	"stpy_scaled_points_t": (_i32, [_i32, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _i64, _i32, _vp]),
	"stpy_lml_grad_reduce": (_i32, [_i32, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
	"stpy_lml_grad_reduce_centred": (_i32, [_i32, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
	"stpy_lml_grad_cov_reduce": (_i32, [_i32, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _vp]),
	"stpy_lml_batch_max_n": (_i64, []),
	"stpy_lml_batch_workspace_bytes": (_i64, [_i32, _i64, _i32, _i64]),
	"stpy_lml_batch": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _dbl, _dbl, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
	"stpy_experts_max_n": (_i64, []),
	"stpy_experts_factor_bytes": (_i64, [_i32, _i64, _i64]),
	"stpy_experts_fit_workspace_bytes": (_i64, [_i32, _i64, _i32, _i64]),
	"stpy_experts_fit": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _dbl, _dbl, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _i64,
						 _vp, _vp, _vp, _i64, _vp]),
	"stpy_experts_predict_workspace_bytes": (_i64, [_i32, _i64, _i32, _i64, _i64]),
	"stpy_experts_predict": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _i64, _vp, _dbl, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64,
							 _vp, _i64, _vp]),
	"stpy_experts_combine": (_i32, [_i32, _i64, _i64, _vp, _vp, _i64, _dbl, _vp, _vp, _vp]),
	"stpy_experts_predict_grad_workspace_bytes": (_i64, [_i32, _i64, _i32, _i64, _i64]),
	"stpy_experts_predict_grad": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _i64, _vp, _dbl, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64,
								  _vp, _vp, _i64, _i64, _vp, _i64, _vp]),
	"stpy_experts_combine_grad": (_i32, [_i32, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _dbl, _vp, _vp, _vp, _vp, _i64, _vp]),
	"stpy_experts_route_max_k": (_i64, []),
	"stpy_experts_centroids": (_i32, [_i32, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
	"stpy_experts_route": (_i32, [_i32, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp]),
	"stpy_experts_predict_routed_workspace_bytes": (_i64, [_i32, _i64, _i32, _i64]),
	"stpy_experts_predict_routed": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _i64, _vp, _dbl, _vp, _i64, _vp, _vp, _vp, _i64, _i64,
										_i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp]),
	"stpy_experts_predict_routed_grad_workspace_bytes": (_i64, [_i32, _i64, _i32, _i64]),
	"stpy_experts_predict_routed_grad": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _i64, _vp, _dbl, _vp, _i64, _vp, _vp, _vp, _i64, _i64,
											 _i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _vp]),
	"stpy_pchol_workspace_bytes": (_i64, [_i32, _i64, _i32, _i64]),
	"stpy_pchol": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _i64, _dbl, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
	"stpy_kmv_workspace_bytes": (_i64, [_i32, _i64, _i64, _i32, _i64]),
	"stpy_kmv": (_i32, [_i32, _i32, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _dbl, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp]),
	"stpy_pcg_workspace_bytes": (_i64, [_i32, _i64, _i32, _i64, _i64]),
	"stpy_pcg": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _dbl, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _dbl, _i32, _i32,
						_vp, _vp, _vp, _vp, _i64, _vp]),
	"stpy_pcg_lanczos": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _dbl, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _dbl, _i32, _i32,
								_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
	"stpy_kmv_dtheta_workspace_bytes": (_i64, [_i32, _i64, _i32, _i64]),
	"stpy_kmv_dtheta": (_i32, [_i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp]),
	"stpy_kmv_dx_workspace_bytes": (_i64, [_i32, _i64, _i64, _i32, _i64]),
	"stpy_kmv_dx": (_i32, [_i32, _i32, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp]),
	"stpy_kmv_dxx_workspace_bytes": (_i64, [_i32, _i64, _i64, _i32, _i64]),
	"stpy_kmv_dxx": (_i32, [_i32, _i32, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp]),
	"stpy_gram_grad_workspace_bytes": (_i64, [_i32, _i64, _i64, _i32, _i32]),
	"stpy_gram_grad": (_i32, [_i32, _i32, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _dbl, _vp, _vp, _vp, _i64, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _i64, _vp]),
	"stpy_trsm_ln_factor": (_i32, [_i32, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
	"stpy_trsm_right_ln": (_i32, [_i32, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _i64, _vp]),
	"stpy_rff_workspace_bytes": (_i64, [_i32, _i64, _i32, _i64]),
	"stpy_rff_embed": (_i32, [_i32, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _vp, _vp, _dbl, _vp, _i64, _i32, _vp, _i64, _vp]),
	"stpy_rff_grad_workspace_bytes": (_i64, [_i32, _i64, _i32, _i64, _i32]),
	"stpy_rff_grad": (_i32, [_i32, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _vp, _vp, _dbl, _vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
	"stpy_profile_enable": (None, [_i32]),
	"stpy_async_status": (_i32, [_vp]),
	"stpy_profile_read_union": (_i32, [_i32, _c.POINTER(_dbl), _c.POINTER(_dbl), _c.POINTER(_i64)]),
	"stpy_tune": (None, [_i32, _i32]),
	"stpy_tune_get": (_i32, [_i32]),
	"stpy_profile_read": (_i32, [_i32, _c.POINTER(_dbl), _c.POINTER(_dbl), _c.POINTER(_i64)]),
}

_lib = None


class StpyHipError(RuntimeError):
	pass


def load():
	"""Load (once) and return the ctypes handle; raises if the HIP library has not been built."""
	global _lib
	if _lib is not None:
		return _lib
	if not os.path.exists(LIB_PATH):
		raise StpyHipError(
			"libstpy_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
			"or `make -C stpy_amd/csrc`. stpy_amd has no CPU fallback." % LIB_PATH)
	lib = ctypes.CDLL(LIB_PATH)
	for name, (res, args) in SIGNATURES.items():
		fn = getattr(lib, name)          # AttributeError here = header/library mismatch
		fn.restype = res
		fn.argtypes = args
	_lib = lib
	return lib


def check(rc, what):
	if rc != 0:
		msg = load().stpy_last_error_string().decode("utf-8", "replace")
		raise StpyHipError("%s failed (rc=%d): %s" % (what, rc, msg))


def check_async(what, stream=None):
	"""Read (and clear) the sticky device error word of the calling stream -- waits for the stream.  Raises StpyHipError when a
	hand-off wait of the one-launch vector solve gave up (its output is NaN from the affected block on)."""
	rc = load().stpy_async_status(stream_ptr() if stream is None else stream)
	if rc != 0:
		raise StpyHipError("%s: device-side failure reported by stpy_async_status (code %d%s)" % (
			what, rc, ": a hand-off wait of the one-launch vector solve timed out, its result is NaN" if rc == 1 else ""))


def device():
	"""The ROCm device this process computes on (one process per GPU: LOCAL_RANK picks it)."""
	if not torch.cuda.is_available():
		raise StpyHipError("stpy_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path.")
	return torch.device("cuda", torch.cuda.current_device())


def stream_ptr():
	return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(dt):
	if dt == torch.float64:
		return F64
	if dt == torch.float32:
		return F32
	raise StpyHipError("unsupported dtype %s (float64 or float32)" % dt)


def ptr(t):
	return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def ld(t):
	"""Leading dimension (elements) of a row-major 2-D tensor: stride(0).  A one-row tensor may report a stride(0) below its row length
	(``x.T.contiguous()`` of an (n, 1) tensor keeps stride 1): it gets the row length instead."""
	return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), int(t.shape[1]), 1)


def to_device(t, dtype=None):
	"""Caller tensor (CPU or GPU, torch or numpy) -> contiguous 2-D/1-D tensor on this process's GPU."""
	if not torch.is_tensor(t):
		t = torch.as_tensor(t)
	dev = device()
	if dtype is None:
		dtype = t.dtype if t.dtype in (torch.float32, torch.float64) else torch.float64
	t = t.to(device=dev, dtype=dtype)
	if t.dim() == 2 and t.stride(1) != 1:
		t = t.contiguous()
	elif t.dim() != 2:
		t = t.contiguous()
	return t


def like_input(result, ref):
	"""Results live where the caller's inputs live (CPU in -> CPU out), as in the reference."""
	if torch.is_tensor(ref) and ref.is_cuda:
		return result
	return result.cpu()


# ---------------------------------------------------------------------------------------------------------------------------
# Typed wrappers, one per launch entry point the package uses.  Each takes torch tensors; derives the dtype code, the dimensions,
# the leading dimensions and the stream (read at call time: the block-cyclic code launches from side streams); allocates the
# workspace the matching query asks for, alive for the call only unless the caller passes a buffer it keeps; and checks the return
# code under the entry point's name.  Arguments that select a kernel route (nb, flags, workspace, mode, lower_only) are the
# caller's.  Nothing here waits for the device.

def _launch(name, *args):
	check(getattr(load(), name)(*args, stream_ptr()), name)


def _work(nbytes, like):
	return torch.empty((int(nbytes),), dtype=torch.uint8, device=like.device)


def _ncols(x, cols):
	"""Coordinates a kernel reads: the ones listed in the device int32 array ``cols``, else every column of x."""
	return x.shape[1] if cols is None else cols.numel()


def gram_workspace(n, q, d, like):
	"""Scratch of stpy_gram for n x q points of d coordinates (one buffer can serve several launches)."""
	return _work(load().stpy_gram_workspace_bytes(dtype_code(like.dtype), n, q, d), like)


def gram(kind, a, b, out, inv_ls, cols=None, kappa=1.0, offset=0.0, diag_add=0.0, lower_only=False, combine=OUT_SET, work=None):
	"""out[j, i] (combine)= k(a_i, b_j) + diag_add [i == j]; out: (|b|, |a|), may be a view."""
	n, q, d = a.shape[0], b.shape[0], _ncols(a, cols)
	work = gram_workspace(n, q, d, out) if work is None else work
	_launch("stpy_gram", kind, dtype_code(out.dtype), ptr(a), n, ld(a), ptr(b), q, ld(b), d, ptr(cols), ptr(inv_ls), kappa, offset, diag_add,
			int(lower_only), combine, ptr(out), ld(out), ptr(work), work.numel())


def gram_diag(kind, x, out, inv_ls, cols=None, kappa=1.0, offset=0.0, combine=OUT_SET, d=None):
	"""out[i] (combine)= k(x_i, x_i).  d: coordinates read (default as gram; 0 for a kernel whose diagonal does not depend on x)."""
	_launch("stpy_gram_diag", kind, dtype_code(out.dtype), ptr(x), x.shape[0], ld(x), _ncols(x, cols) if d is None else d, ptr(cols), ptr(inv_ls),
			kappa, offset, combine, ptr(out))


def gram_grad(kind, x, xt, G, inv_ls, cols=None, kappa=1.0, offset=0.0, alpha=None, u=None, Wt=None, v=None, combine=OUT_SET, H=None):
	"""G[t] (combine)= d/dxt_t sum_i (u_t alpha_i + v_t Wt[t, i]) k(xt_t, x_i); with H also the second derivatives."""
	m, n, d = xt.shape[0], x.shape[0], _ncols(x, cols)
	order = 1 if H is None else 2
	work = _work(load().stpy_gram_grad_workspace_bytes(dtype_code(G.dtype), m, n, d, order), G)
	_launch("stpy_gram_grad", kind, dtype_code(G.dtype), ptr(x), n, ld(x), ptr(xt), m, ld(xt), d, ptr(cols), ptr(inv_ls), float(kappa), float(offset),
			ptr(alpha), ptr(u), ptr(Wt), ld(Wt) if Wt is not None else 0, ptr(v), order, combine, ptr(G), ld(G), ptr(H), ptr(work), work.numel())


def combine(out, src, op=OUT_SET, diag_add=0.0):
	"""out (op)= src elementwise, then + diag_add on the diagonal; src may be out."""
	_launch("stpy_combine", dtype_code(out.dtype), out.shape[0], out.shape[1], ptr(out), ld(out), ptr(src), ld(src), op, diag_add)


def gemm_nt(A, B, C, mode=0, lower_only=False):
	"""C (mode 0: =, 1: -=, 2: +=) A B^T."""
	_launch("stpy_gemm_nt", dtype_code(C.dtype), A.shape[0], B.shape[0], A.shape[1], ptr(A), ld(A), ptr(B), ld(B), ptr(C), ld(C), mode, int(lower_only))


def gemm_nt_splitk_passes(A, B):
	"""K passes the library recommends for A B^T (1: gemm_nt)."""
	return int(load().stpy_gemm_nt_splitk_passes(A.shape[0], B.shape[0], A.shape[1]))


def gemm_nt_splitk(A, B, C, mode, passes, work):
	"""gemm_nt in ``passes`` K pieces summed in a fixed order; work: at least passes * |A| * |B| elements."""
	_launch("stpy_gemm_nt_splitk", dtype_code(C.dtype), A.shape[0], B.shape[0], A.shape[1], ptr(A), ld(A), ptr(B), ld(B), ptr(C), ld(C), mode,
			passes, ptr(work), work.numel() * work.element_size())


def gemm_nt_bc(A, B, C, mode, bc):
	"""gemm_nt on a window of a block-cyclic local matrix; bc = (nb_dist, pr, pc, myr, myc, i0, j0)."""
	_launch("stpy_gemm_nt_bc", dtype_code(C.dtype), A.shape[0], B.shape[0], A.shape[1], ptr(A), ld(A), ptr(B), ld(B), ptr(C), ld(C), mode,
			*[int(v) for v in bc])


def syrk(A, C, mode=0):
	"""C (mode) A A^T on the lower tiles, with a workspace where the library has a use for one."""
	n, k = A.shape
	wb = int(load().stpy_syrk_workspace_bytes(dtype_code(C.dtype), n, k))
	work = _work(wb, C) if wb > 0 else None
	_launch("stpy_syrk", dtype_code(C.dtype), n, k, ptr(A), ld(A), ptr(C), ld(C), mode, ptr(work), wb)


def potrf_winv_elems(n):
	return int(load().stpy_potrf_winv_elems(n))


def potrf(A, nb=0, flags=0):
	"""In-place Cholesky of the square view A.  Returns (winv, info): the inverse diagonal blocks and the device status word (first
	failing pivot, 1-based), unread -- the caller decides when to wait for it."""
	n = A.shape[0]
	winv = torch.empty((potrf_winv_elems(n),), dtype=A.dtype, device=A.device)
	work = _work(load().stpy_potrf_workspace_bytes(dtype_code(A.dtype), n, nb), A)
	info = torch.zeros((1,), dtype=torch.int32, device=A.device)
	_launch("stpy_potrf", dtype_code(A.dtype), n, ptr(A), ld(A), ptr(winv), winv.numel(), ptr(work), work.numel(), nb, flags, ptr(info))
	return winv, info


def potrf_append(A, n0, winv, z, y):
	"""Extends the factor in rows [0, n0) of A by len(y) rows, z from L^-1 y_old to L^-1 y (layout: stpy_potrf_append in the header).
	Returns the unread status word, as potrf."""
	k = y.shape[0]
	work = _work(max(int(load().stpy_potrf_append_workspace_bytes(dtype_code(A.dtype), n0, k)), 1), A)
	info = torch.zeros((1,), dtype=torch.int32, device=A.device)
	_launch("stpy_potrf_append", dtype_code(A.dtype), n0, k, ptr(A), ld(A), ptr(winv), winv.numel(), ptr(z), ptr(y), ptr(work), work.numel(), ptr(info))
	return info


def chol_update(L, winv, W, sign=1):
	"""Rank-k update (sign = +1) or downdate (-1) of a factor in place: L L^T + sign W W^T, winv refreshed (stpy_chol_update in the header).
	W, (n, k) with rows of k contiguous elements, is destroyed.  Returns the unread status word, as potrf."""
	n, k = L.shape[0], W.shape[1]
	work = _work(max(int(load().stpy_chol_update_workspace_bytes(dtype_code(L.dtype), n, k)), 1), L)
	info = torch.zeros((1,), dtype=torch.int32, device=L.device)
	_launch("stpy_chol_update", dtype_code(L.dtype), n, k, int(sign), ptr(L), ld(L), ptr(winv), winv.numel(), ptr(W), ld(W), ptr(work), work.numel(), ptr(info))
	return info


def potrf_delete(A, n0, idx, B, winv):
	"""The factor of order n0 in A without the rows / columns ``idx`` (strictly increasing ints in [0, n0)), compacted into the
	different buffer B with its inverse diagonal blocks in winv (layout: stpy_potrf_delete in the header).  The indices travel as a
	host array, which the library validates and has read when the call returns (it passes them on as kernel arguments).  Returns the unread status word, as potrf."""
	k = len(idx)
	dt = dtype_code(A.dtype)
	host = (_c.c_int32 * max(k, 1))(*idx)
	work = _work(max(int(load().stpy_potrf_delete_workspace_bytes(dt, n0, k)), 1), A)
	info = torch.zeros((1,), dtype=torch.int32, device=A.device)
	_launch("stpy_potrf_delete", dt, n0, k, host, ptr(A), ld(A), ptr(B), ld(B), ptr(winv), winv.numel(), ptr(work), work.numel(), ptr(info))
	return info


def potri(L, winv, n=None, work=None):
	"""(L L^T)^-1, full symmetric: the leading n x n block (default: all) of a new matrix of L's order.  work: scratch of that size,
	allocated here unless the caller keeps one."""
	N = L.shape[0]
	Kinv = torch.empty((N, N), dtype=L.dtype, device=L.device)
	work = torch.empty((N, N), dtype=L.dtype, device=L.device) if work is None else work
	_launch("stpy_potri", dtype_code(L.dtype), N, ptr(L), ld(L), ptr(winv), winv.numel(), ptr(Kinv), ld(Kinv), ptr(work),
			work.numel() * work.element_size())
	Kinv = Kinv[:n, :n]
	symmetrize_lower(Kinv)
	return Kinv


def _trsm(name, B, L, winv, nb, flags, workspace):
	m, n = B.shape
	work = _work(load().stpy_trsm_workspace_bytes(dtype_code(B.dtype), m, n, nb), B) if workspace else None
	_launch(name, dtype_code(B.dtype), m, n, ptr(L), ld(L), ptr(winv), winv.numel(), ptr(B), ld(B), nb, flags, ptr(work), 0 if work is None else work.numel())


def trsm_right_lt(B, L, winv, nb=0, flags=0, workspace=False):
	"""B <- B L^-T in place.  ``workspace`` selects the algorithm: with one, large solves may run left-looking with K passes."""
	_trsm("stpy_trsm_right_lt", B, L, winv, nb, flags, workspace)


def trsm_right_ln(B, Lr, winvr, nb=0, flags=0, workspace=False):
	"""B <- B L^-1 in place, from the reversed factor of trsm_ln_factor."""
	_trsm("stpy_trsm_right_ln", B, Lr, winvr, nb, flags, workspace)


def trsm_ln_factor(L, winv):
	"""(Lr, winvr): the reversed factor J L^T J and its inverse diagonal blocks."""
	Lr, winvr = torch.empty_like(L), torch.empty_like(winv)
	_launch("stpy_trsm_ln_factor", dtype_code(L.dtype), L.shape[0], ptr(L), ld(L), ptr(winv), winv.numel(), ptr(Lr), ld(Lr), ptr(winvr))
	return Lr, winvr


def trsv(L, winv, rhs, trans=0):
	"""L^-1 rhs (trans = 0) or L^-T rhs (trans = 1), a vector of L's order; rhs, zero-padded to that order, is left as it is."""
	n = L.shape[0]
	rhs = rhs.reshape(-1)
	if rhs.numel() == n:
		y = rhs.clone()
	else:
		y = torch.zeros((n,), dtype=L.dtype, device=L.device)
		y[:rhs.numel()] = rhs
	out = torch.empty_like(y)
	_launch("stpy_trsv", dtype_code(L.dtype), n, ptr(L), ld(L), ptr(winv), winv.numel(), ptr(y), ptr(out), trans)          # (y: scratch)
	return out


def predict(X, z, mu=None, sigma=None, kdiag=None, clamp=0):
	"""mu[i] = <X_i, z>, sigma[i] = sqrt(kdiag[i] - <X_i, X_i>) (clamp 1: clamped at 0; 2: sigma[i] = <X_i, X_i>); either may be None."""
	_launch("stpy_predict", dtype_code(X.dtype), X.shape[0], X.shape[1], ptr(X), ld(X), ptr(z), ptr(kdiag), ptr(mu), ptr(sigma), clamp)


def predict_finish(mu=None, sumsq=None, kdiag=None, scale=1.0, sigma=None, clamp=0):
	"""mu *= scale in place, sigma = sqrt(kdiag - scale * sumsq); either may be None."""
	t = mu if mu is not None else sigma
	_launch("stpy_predict_finish", dtype_code(t.dtype), t.shape[0], ptr(mu), ptr(sumsq), ptr(kdiag), scale, ptr(sigma), clamp)


def logdet_quad(L, z=None):
	"""[sum_i log L_ii, z^T z] (z None: 0), a 2-element device tensor."""
	out2 = torch.empty((2,), dtype=L.dtype, device=L.device)
	_launch("stpy_logdet_quad", dtype_code(L.dtype), L.shape[0], ptr(L), ld(L), ptr(z), ptr(out2))
	return out2


def trace_dot(A=None, u=None, v=None):
	"""[tr(A), <u, v>] (A or u None: 0) in a fixed summation order, a 2-element device tensor."""
	t = A if A is not None else u
	out2 = torch.empty((2,), dtype=t.dtype, device=t.device)
	_launch("stpy_trace_dot", dtype_code(t.dtype), t.shape[0], ptr(A), ld(A) if A is not None else 0, ptr(u), ptr(v), ptr(out2))
	return out2


def tril(A):
	_launch("stpy_tril", dtype_code(A.dtype), A.shape[0], ptr(A), ld(A))


def symmetrize_lower(A):
	_launch("stpy_symmetrize_lower", dtype_code(A.dtype), A.shape[0], ptr(A), ld(A))


def scaled_points_t(x, inv_ls, cols=None, centre=False):
	"""[Xs | 1]^T, (d + 1, n): the rows of x[:, cols] * inv_ls as columns, then a row of ones.  centre: coordinates relative to x[0] (the
	operand lml_grad_reduce(centred=True) expects)."""
	n, d = x.shape[0], _ncols(x, cols)
	out = torch.empty((d + 1, n), dtype=x.dtype, device=x.device)
	_launch("stpy_scaled_points_t", dtype_code(x.dtype), ptr(x), n, ld(x), d, ptr(cols), ptr(inv_ls), ptr(out), ld(out), 3 if centre else 1)
	return out


def lml_weight(kind, x, inv_ls, kappa, weight, alpha, Kinv, H, cols=None):
	"""H = (weight Kinv - alpha alpha^T) o F, F the lengthscale-derivative factor of one kernel term; H may be Kinv."""
	n, d = x.shape[0], _ncols(x, cols)
	work = gram_workspace(n, n, d, x)
	_launch("stpy_lml_weight", kind, dtype_code(x.dtype), ptr(x), n, ld(x), d, ptr(cols), ptr(inv_ls), kappa, weight, ptr(alpha), ptr(Kinv), ld(Kinv),
			ptr(H), ld(H), ptr(work), work.numel())


def lml_grad_reduce(x, inv_ls, P, pidx, acc, cols=None, centred=False):
	"""acc[pidx[k]] += inv_ls[k] / 2 sum_ij H_ij (xs_ik - xs_jk)^2 from P = H [Xs | 1]; centred: P = H [Xs - xs_0 | 1] (scaled_points_t(centre=True))."""
	_launch("stpy_lml_grad_reduce_centred" if centred else "stpy_lml_grad_reduce", dtype_code(x.dtype), ptr(x), x.shape[0], ld(x), _ncols(x, cols), ptr(cols),
			ptr(inv_ls), ptr(P), ld(P), ptr(pidx), ptr(acc))


def lml_grad_cov_reduce(x, z, P, out, cols=None):
	_launch("stpy_lml_grad_cov_reduce", dtype_code(x.dtype), ptr(x), x.shape[0], ld(x), _ncols(x, cols), ptr(cols), ptr(z), ld(z), z.shape[1], ptr(P),
			ld(P), ptr(out))


def lml_batch_max_n():
	"""Largest n the batched evidence kernel accepts."""
	return int(load().stpy_lml_batch_max_n())


def lml_batch(kind, x, y, inv_ls, noise, pidx, n_params, kappa, weight, cols=None):
	"""Evidence value and gradient of ``B = inv_ls.shape[0]`` candidates on the same data in one launch (stpy_lml_batch in the header).
	inv_ls (B, d), noise (B,) float64 and pidx (d,) int32 on the device.  Returns (value (B,), grad (B, n_params + 1), info (B,) int32,
	packed): views of ONE device buffer ``packed`` (bytes), so that a caller fetches all three with a single copy."""
	n, d, B = x.shape[0], _ncols(x, cols), inv_ls.shape[0]
	ldg = n_params + 1
	packed = torch.empty((B * (ldg + 1) * 8 + B * 4,), dtype=torch.uint8, device=x.device)
	value = packed[:B * 8].view(torch.float64)
	grad = packed[B * 8:B * (ldg + 1) * 8].view(torch.float64).view(B, ldg)
	info = packed[B * (ldg + 1) * 8:].view(torch.int32)
	work = _work(max(int(load().stpy_lml_batch_workspace_bytes(dtype_code(x.dtype), n, d, B)), 16), x)
	_launch("stpy_lml_batch", kind, dtype_code(x.dtype), ptr(x), n, ld(x), d, ptr(cols), ptr(y), B, ptr(inv_ls), ld(inv_ls), ptr(noise),
			float(kappa), float(weight), ptr(pidx), int(n_params), ptr(value), ptr(grad), ldg, ptr(info), ptr(work), work.numel())
	return value, grad, info, packed


def experts_max_n():
	"""Largest expert stpy_experts_fit accepts."""
	return int(load().stpy_experts_max_n())


def experts_factor(nmax, E, like):
	"""The factor buffer of E experts of at most nmax points (bytes; stpy_experts_factor_bytes): written by experts_fit, read by experts_predict."""
	return _work(max(int(load().stpy_experts_factor_bytes(F64, nmax, E)), 16), like)


def experts_fit_workspace(nmax, d, E, like):
	"""Scratch of stpy_experts_fit (dead after the call; one buffer can serve several launches)."""
	return _work(max(int(load().stpy_experts_fit_workspace_bytes(F64, nmax, d, E)), 16), like)


def experts_fit(kind, xs, ys, offsets, nmax, inv_ls, noise, kappa, weight, factor, alpha, pidx=None, n_params=0, cols=None, work=None):
	"""E = offsets.numel() - 1 exact GPs on the row blocks offsets[e] .. offsets[e + 1] of xs / ys in one launch, plus one for the totals
	(stpy_experts_fit in the header).  inv_ls (d,), noise (1,) float64 and offsets (E + 1,) int32 on the device; ``factor`` (experts_factor) and
	``alpha`` (N,) are written.  With ``pidx`` (d,) int32 the gradient is computed: n_params lengthscale slots, then the noise std.  Returns
	(value (E,), grad (E, n_params + 1) or None, total (n_params + 2,) or (1,), info (E,) int32, packed): views of ONE device buffer ``packed``
	(bytes: [total | value | grad | info]), so that a caller fetches all of them with a single copy."""
	N, d, E = xs.shape[0], _ncols(xs, cols), offsets.numel() - 1
	ldg = n_params + 1 if pidx is not None else 0
	nt = n_params + 2 if pidx is not None else 1
	packed = torch.empty(((nt + E * (1 + ldg)) * 8 + E * 4,), dtype=torch.uint8, device=xs.device)
	total = packed[:nt * 8].view(torch.float64)
	value = packed[nt * 8:(nt + E) * 8].view(torch.float64)
	grad = packed[(nt + E) * 8:(nt + E * (1 + ldg)) * 8].view(torch.float64).view(E, ldg) if pidx is not None else None
	info = packed[(nt + E * (1 + ldg)) * 8:].view(torch.int32)
	work = experts_fit_workspace(nmax, d, E, xs) if work is None else work
	_launch("stpy_experts_fit", kind, dtype_code(xs.dtype), ptr(xs), N, ld(xs), d, ptr(cols), ptr(ys), ptr(offsets), E, int(nmax), ptr(inv_ls), ptr(noise),
			float(kappa), float(weight), ptr(pidx), int(n_params), ptr(factor), factor.numel(), ptr(alpha), ptr(value), ptr(grad), ldg, ptr(total), ptr(info),
			ptr(work), work.numel())
	return value, grad, total, info, packed


def experts_predict(kind, xs, offsets, nmax, inv_ls, kappa, factor, alpha, info, xt, mu_e, var_e, cols=None, work=None):
	"""mu_e[e, t], var_e[e, t] (E x M, row stride ld): every expert's posterior mean and latent variance at the test points xt, one launch
	(stpy_experts_predict in the header)."""
	N, d, E, M = xs.shape[0], _ncols(xs, cols), offsets.numel() - 1, xt.shape[0]
	if work is None:
		work = _work(max(int(load().stpy_experts_predict_workspace_bytes(F64, int(nmax), d, E, M)), 16), xs)
	_launch("stpy_experts_predict", kind, dtype_code(xs.dtype), ptr(xs), N, ld(xs), d, ptr(cols), ptr(offsets), E, int(nmax), ptr(inv_ls), float(kappa),
			ptr(factor), factor.numel(), ptr(alpha), ptr(info), ptr(xt), M, ld(xt), ptr(mu_e), ptr(var_e), ld(mu_e), ptr(work), work.numel())


def experts_combine(mode, mu_e, var_e, kappa, mu, var):
	"""mu, var (M,) from the experts' (E, M) predictions: mode 0 PoE, 1 gPoE, 2 BCM, 3 rBCM (stpy_experts_combine in the header)."""
	_launch("stpy_experts_combine", int(mode), mu_e.shape[0], mu_e.shape[1], ptr(mu_e), ptr(var_e), ld(mu_e), float(kappa), ptr(mu), ptr(var))


def _grad_strides(g):
	"""(ldg, lde) of an (E, M, d) gradient array with unit last stride, which may be a view: row and expert stride in elements (a dimension of
	one entry may report any stride: it gets the dense one)."""
	E, M, d = g.shape
	if d > 1 and g.stride(2) != 1:
		raise StpyHipError("experts gradients: the last dimension must be contiguous")
	ldg = g.stride(1) if M > 1 else max(g.stride(1), d, 1)
	return ldg, (g.stride(0) if E > 1 else max(g.stride(0), M * ldg, 1))


def experts_predict_grad_workspace(nmax, d, E, M, like):
	"""Scratch of stpy_experts_predict_grad (dead after the call; one buffer can serve several launches of at most these sizes)."""
	return _work(max(int(load().stpy_experts_predict_grad_workspace_bytes(F64, int(nmax), d, E, M)), 16), like)


def experts_predict_grad(kind, xs, offsets, nmax, inv_ls, kappa, factor, alpha, info, xt, mu_e, var_e, gmu_e, gvar_e, cols=None, work=None):
	"""experts_predict plus the input gradients gmu_e, gvar_e (E, M, d) of every expert's mean and latent variance over the selected coordinates,
	one launch (stpy_experts_predict_grad in the header); mu_e and var_e carry the bits of experts_predict."""
	N, d, E, M = xs.shape[0], _ncols(xs, cols), offsets.numel() - 1, xt.shape[0]
	if work is None:
		work = experts_predict_grad_workspace(nmax, d, E, M, xs)
	ldg, lde = _grad_strides(gmu_e)
	if (ldg, lde) != _grad_strides(gvar_e):
		raise StpyHipError("experts_predict_grad: gmu_e and gvar_e must share their strides")
	_launch("stpy_experts_predict_grad", kind, dtype_code(xs.dtype), ptr(xs), N, ld(xs), d, ptr(cols), ptr(offsets), E, int(nmax), ptr(inv_ls), float(kappa),
			ptr(factor), factor.numel(), ptr(alpha), ptr(info), ptr(xt), M, ld(xt), ptr(mu_e), ptr(var_e), ld(mu_e), ptr(gmu_e), ptr(gvar_e), ldg, lde,
			ptr(work), work.numel())


def experts_combine_grad(mode, mu_e, var_e, gmu_e, gvar_e, kappa, mu, var, dmu, dstd):
	"""experts_combine plus dmu, dstd (M, d): the input gradients of the combined mean and standard deviation by the chain rule through the
	combination, its clamp and rBCM's weights (stpy_experts_combine_grad in the header)."""
	ldg, lde = _grad_strides(gmu_e)
	if (ldg, lde) != _grad_strides(gvar_e) or ld(dmu) != ld(dstd):
		raise StpyHipError("experts_combine_grad: gmu_e / gvar_e and dmu / dstd must share their strides")
	_launch("stpy_experts_combine_grad", int(mode), mu_e.shape[0], mu_e.shape[1], gmu_e.shape[2], ptr(mu_e), ptr(var_e), ld(mu_e), ptr(gmu_e), ptr(gvar_e),
			ldg, lde, float(kappa), ptr(mu), ptr(var), ptr(dmu), ptr(dstd), ld(dmu))


def experts_route_max_k():
	"""Largest k stpy_experts_route selects."""
	return int(load().stpy_experts_route_max_k())


def experts_centroids(xs, offsets, inv_ls, cols=None):
	"""cent (E, d): every expert's mean point in scaled coordinates x[cols] * inv_ls, +inf for an expert without rows; one launch
	(stpy_experts_centroids in the header)."""
	N, d, E = xs.shape[0], _ncols(xs, cols), offsets.numel() - 1
	cent = torch.empty((E, d), dtype=torch.float64, device=xs.device)
	_launch("stpy_experts_centroids", dtype_code(xs.dtype), ptr(xs), N, ld(xs), d, ptr(cols), ptr(offsets), E, ptr(inv_ls), ptr(cent), ld(cent))
	return cent


def experts_route(cent, inv_ls, xt, k, cols=None):
	"""sel (M, k) int32: the k experts whose centroids are nearest to every test point, ties to the lower id, each row ascending in expert id;
	one launch (stpy_experts_route in the header)."""
	E, d, M = cent.shape[0], cent.shape[1], xt.shape[0]
	sel = torch.empty((M, int(k)), dtype=torch.int32, device=xt.device)
	_launch("stpy_experts_route", dtype_code(cent.dtype), ptr(cent), ld(cent), E, d, ptr(cols), ptr(inv_ls), ptr(xt), M, ld(xt), int(k), ptr(sel))
	return sel


def experts_route_tiles(E, M, k):
	"""The host-side bound on the tiles of a routed work list: floor(M k / 32) + min(E, M k)."""
	return (int(M) * int(k)) // 32 + min(int(E), int(M) * int(k))


def experts_work_list(sel, E):
	"""(wexp (T,), wpair (32 T,)) int32, T = experts_route_tiles: the work list of a routed prediction from sel (M, k), built on the device with
	integer tensor operations and no read-back.  The pair ids p = t k + j, stably sorted by expert (so test points ascend within an expert), are
	cut into tiles of 32 per expert; unused tiles carry expert -1, empty columns pair -1."""
	M, k = sel.shape
	P, T, dev = M * k, experts_route_tiles(E, M, k), sel.device
	e = sel.reshape(-1).long()
	order = torch.argsort(e, stable=True)
	cnt = torch.zeros((E,), dtype=torch.int64, device=dev).scatter_add_(0, e, torch.ones_like(e))
	tiles = (cnt + 31) // 32
	tstart, pstart = torch.cumsum(tiles, 0) - tiles, torch.cumsum(cnt, 0) - cnt
	es = e[order]
	rank = torch.arange(P, dtype=torch.int64, device=dev) - pstart[es]
	tile = tstart[es] + rank // 32
	wexp = torch.full((T,), -1, dtype=torch.int32, device=dev)
	wpair = torch.full((T * 32,), -1, dtype=torch.int32, device=dev)
	wexp[tile] = es.int()
	wpair[tile * 32 + rank % 32] = order.int()
	return wexp, wpair


def experts_predict_routed_workspace(nmax, d, T, like, grad=False):
	"""Scratch of stpy_experts_predict_routed (grad: of _predict_routed_grad) for a work list of T tiles; dead after the call."""
	query = load().stpy_experts_predict_routed_grad_workspace_bytes if grad else load().stpy_experts_predict_routed_workspace_bytes
	return _work(max(int(query(F64, int(nmax), d, int(T))), 16), like)


def experts_predict_routed(kind, xs, offsets, nmax, inv_ls, kappa, factor, alpha, info, xt, wexp, wpair, mu_s, var_s, cols=None, work=None):
	"""mu_s[j, t], var_s[j, t] (k x M, row stride ld): the prediction of the expert in slot j of test point t's selection, for the pairs the work
	list (experts_work_list) holds; one launch (stpy_experts_predict_routed in the header)."""
	N, d, E, M, k, T = xs.shape[0], _ncols(xs, cols), offsets.numel() - 1, xt.shape[0], mu_s.shape[0], wexp.numel()
	if work is None:
		work = experts_predict_routed_workspace(nmax, d, T, xs)
	_launch("stpy_experts_predict_routed", kind, dtype_code(xs.dtype), ptr(xs), N, ld(xs), d, ptr(cols), ptr(offsets), E, int(nmax), ptr(inv_ls), float(kappa),
			ptr(factor), factor.numel(), ptr(alpha), ptr(info), ptr(xt), M, ld(xt), k, ptr(wexp), ptr(wpair), T, ptr(mu_s), ptr(var_s), ld(mu_s),
			ptr(work), work.numel())


def experts_predict_routed_grad(kind, xs, offsets, nmax, inv_ls, kappa, factor, alpha, info, xt, wexp, wpair, mu_s, var_s, gmu_s, gvar_s, cols=None, work=None):
	"""experts_predict_routed plus the input gradients gmu_s, gvar_s (k, M, d) over the selected coordinates, one launch
	(stpy_experts_predict_routed_grad in the header)."""
	N, d, E, M, k, T = xs.shape[0], _ncols(xs, cols), offsets.numel() - 1, xt.shape[0], mu_s.shape[0], wexp.numel()
	if work is None:
		work = experts_predict_routed_workspace(nmax, d, T, xs, grad=True)
	ldg, lde = _grad_strides(gmu_s)
	if (ldg, lde) != _grad_strides(gvar_s):
		raise StpyHipError("experts_predict_routed_grad: gmu_s and gvar_s must share their strides")
	_launch("stpy_experts_predict_routed_grad", kind, dtype_code(xs.dtype), ptr(xs), N, ld(xs), d, ptr(cols), ptr(offsets), E, int(nmax), ptr(inv_ls),
			float(kappa), ptr(factor), factor.numel(), ptr(alpha), ptr(info), ptr(xt), M, ld(xt), k, ptr(wexp), ptr(wpair), T, ptr(mu_s), ptr(var_s),
			ld(mu_s), ptr(gmu_s), ptr(gvar_s), ldg, lde, ptr(work), work.numel())


def pchol(kind, x, inv_ls, m, cols=None, kappa=1.0, tol=0.0, ldf=None):
	"""Greedy pivoted partial Cholesky of the kernel matrix of the rows of x (stpy_pchol in the header), at most m steps.  Returns
	(piv (m,) int32, Ft (m, n), dres (n,), rank (1,) int32), all on the device and unread: rows of Ft and entries of piv from the rank on
	are 0 / -1.  ldf: row stride of Ft's storage (default n), of which Ft is the first n columns."""
	n, d = x.shape[0], _ncols(x, cols)
	Ft = torch.empty((m, n if ldf is None else int(ldf)), dtype=x.dtype, device=x.device)[:, :n]
	dres = torch.empty((n,), dtype=x.dtype, device=x.device)
	piv = torch.empty((m,), dtype=torch.int32, device=x.device)
	rank = torch.empty((1,), dtype=torch.int32, device=x.device)
	work = _work(load().stpy_pchol_workspace_bytes(dtype_code(x.dtype), n, d, m), x)
	_launch("stpy_pchol", kind, dtype_code(x.dtype), ptr(x), n, ld(x), d, ptr(cols), ptr(inv_ls), float(kappa), m, float(tol), ptr(Ft), ld(Ft),
			ptr(dres), ptr(piv), ptr(rank), ptr(work), work.numel())
	return piv, Ft, dres, rank


def kmv_workspace(n, q, d, t, like):
	"""Scratch of stpy_kmv (the partial sums of a cut j range); one buffer can serve several launches."""
	return _work(load().stpy_kmv_workspace_bytes(dtype_code(like.dtype), n, q, d, t), like)


def kmv(kind, a, b, Vt, Yt, inv_ls, cols=None, kappa=1.0, diag_add=0.0, work=None):
	"""Yt[c, i] = sum_j k(a_i, b_j) Vt[c, j] + diag_add Vt[c, i], the kernel matrix never formed (stpy_kmv in the header).  Vt: (t, |b|),
	Yt: (t, |a|), one right-hand side per row; both may be column windows of wider storage."""
	n, q, d, t = a.shape[0], b.shape[0], _ncols(a, cols), Vt.shape[0]
	work = kmv_workspace(n, q, d, t, Yt) if work is None else work
	_launch("stpy_kmv", kind, dtype_code(Yt.dtype), ptr(a), n, ld(a), ptr(b), q, ld(b), d, ptr(cols), ptr(inv_ls), float(kappa), float(diag_add),
			ptr(Vt), t, ld(Vt), ptr(Yt), ld(Yt), ptr(work), work.numel())


def pcg_workspace(n, d, t, r, like):
	"""State and scratch of stpy_pcg for t columns of n points and a rank-r preconditioner: keep it between the calls of one solve."""
	return _work(load().stpy_pcg_workspace_bytes(dtype_code(like.dtype), n, d, t, r), like)


def pcg(kind, x, inv_ls, Bt, Xt, work, out, cols=None, kappa=1.0, diag_add=0.0, Gt=None, Gn=None, tol=0.0, iters=10, init=True):
	"""``iters`` iterations of block preconditioned CG on (K(x, x) + diag_add I) X_c = B_c, rows of Bt / Xt (t, n) (stpy_pcg in the header).
	``work`` (pcg_workspace) carries the state from call to call; ``out`` = (relres (t,), bx (t,), its (t,) int32), device tensors written
	at the end of the call and unread.  Gt (r, n) / Gn (n, r): the preconditioner I - G G^T, or None."""
	n, d, t = x.shape[0], _ncols(x, cols), Bt.shape[0]
	r = 0 if Gt is None else Gt.shape[0]
	relres, bx, its = out
	_launch("stpy_pcg", kind, dtype_code(Xt.dtype), ptr(x), n, ld(x), d, ptr(cols), ptr(inv_ls), float(kappa), float(diag_add),
			ptr(Gt), ld(Gt) if r else 0, ptr(Gn), ld(Gn) if r else 0, r, ptr(Bt), ld(Bt), ptr(Xt), ld(Xt), t, float(tol), int(iters), int(bool(init)),
			ptr(relres), ptr(bx), ptr(its), ptr(work), work.numel())


def pcg_lanczos(kind, x, inv_ls, Bt, Xt, work, out, coef, rz0, cols=None, kappa=1.0, diag_add=0.0, Gt=None, Gn=None, tol=0.0, iters=10, init=True):
	"""``pcg`` that also records the CG scalars (stpy_pcg_lanczos in the header): coef (t, cap, 2) float64 -- the step length and the direction
	ratio of every iteration, as applied -- and rz0 (t,) float64 = <B_c, M^-1 B_c>, device tensors.  Slots from its[c] on are left as they are."""
	n, d, t = x.shape[0], _ncols(x, cols), Bt.shape[0]
	r = 0 if Gt is None else Gt.shape[0]
	relres, bx, its = out
	if coef.dtype != torch.float64 or rz0.dtype != torch.float64 or not coef.is_contiguous() or coef.shape[0] != t or coef.shape[2] != 2 or rz0.numel() != t:
		raise StpyHipError("pcg_lanczos: coef must be a contiguous float64 (t, cap, 2) tensor and rz0 a float64 (t,) tensor")
	_launch("stpy_pcg_lanczos", kind, dtype_code(Xt.dtype), ptr(x), n, ld(x), d, ptr(cols), ptr(inv_ls), float(kappa), float(diag_add),
			ptr(Gt), ld(Gt) if r else 0, ptr(Gn), ld(Gn) if r else 0, r, ptr(Bt), ld(Bt), ptr(Xt), ld(Xt), t, float(tol), int(iters), int(bool(init)),
			ptr(relres), ptr(bx), ptr(its), ptr(coef), coef.shape[1], ptr(rz0), ptr(work), work.numel())


def kmv_dtheta_workspace(n, d, t, like):
	"""Scratch of stpy_kmv_dtheta (one partial row per workgroup and pair)."""
	return _work(load().stpy_kmv_dtheta_workspace_bytes(dtype_code(like.dtype), n, d, t), like)


def kmv_dtheta(kind, x, inv_ls, Ut, Vt, out, cols=None, kappa=1.0, work=None):
	"""out[c] = (u_c^T (dK / d inv_ls[k]) v_c * inv_ls[k] for k < d, u_c^T K v_c, <u_c, v_c>) for the rows of Ut / Vt (t, n), K = k(x, x) never
	formed (stpy_kmv_dtheta in the header).  out: (t, d + 2), may be a column window of wider storage."""
	n, d, t = x.shape[0], _ncols(x, cols), Ut.shape[0]
	work = kmv_dtheta_workspace(n, d, t, out) if work is None else work
	_launch("stpy_kmv_dtheta", kind, dtype_code(out.dtype), ptr(x), n, ld(x), d, ptr(cols), ptr(inv_ls), float(kappa), ptr(Ut), ld(Ut), ptr(Vt), ld(Vt), t,
			ptr(out), ld(out), ptr(work), work.numel())


def kmv_dx_workspace(n, q, d, t, like):
	"""Scratch of stpy_kmv_dx (the tiles of a cut j range); one buffer can serve several launches of the same shape."""
	return _work(load().stpy_kmv_dx_workspace_bytes(dtype_code(like.dtype), n, q, d, t), like)


def kmv_dx(kind, a, b, Vt, out, inv_ls, cols=None, kappa=1.0, work=None):
	"""out[c, i] = (d/da_i[cols[k]] for k < d, then the value) of sum_j Vt[c, j] k(a_i, b_j), the kernel matrix never formed (stpy_kmv_dx in the
	header).  Vt: (t, |b|), may be a column window of wider storage; out: (t, |a|, >= d + 1) with a unit last stride, may be a window of wider
	storage in both leading dimensions."""
	n, q, d, t = a.shape[0], b.shape[0], _ncols(a, cols), Vt.shape[0]
	if out.dim() != 3 or out.shape[0] != t or out.shape[1] != n or out.shape[2] < d + 1 or out.stride(2) != 1:
		raise StpyHipError("kmv_dx: out must be (t, n, >= d + 1) = (%d, %d, >= %d) with a unit last stride, got %s" % (t, n, d + 1, tuple(out.shape)))
	ldo = out.stride(1) if n > 1 else max(out.stride(1), int(out.shape[2]))
	ldc = out.stride(0) if t > 1 else max(out.stride(0), n * ldo)
	work = kmv_dx_workspace(n, q, d, t, out) if work is None else work
	_launch("stpy_kmv_dx", kind, dtype_code(out.dtype), ptr(a), n, ld(a), ptr(b), q, ld(b), d, ptr(cols), ptr(inv_ls), float(kappa),
			ptr(Vt), ld(Vt), t, ptr(out), ldc, ldo, ptr(work), work.numel())


def kmv_dxx_ncol(d):
	"""Columns of a point in the output of stpy_kmv_dxx: d gradients, the value, the lower triangle of the Hessian row by row."""
	return 1 + d + d * (d + 1) // 2


def kmv_dxx_workspace(n, q, d, t, like):
	"""Scratch of stpy_kmv_dxx (the tiles of a cut j range); does not decrease in n, q or t, so one buffer sized for the largest problem serves all."""
	return _work(load().stpy_kmv_dxx_workspace_bytes(dtype_code(like.dtype), n, q, d, t), like)


def kmv_dxx(kind, a, b, Vt, out, inv_ls, cols=None, kappa=1.0, work=None):
	"""out[c, i] = (d/da_i[cols[k]] for k < d, the value, then d2/da_i[cols[k]] da_i[cols[l]] for l <= k < d at d + 1 + k (k + 1) / 2 + l) of
	sum_j Vt[c, j] k(a_i, b_j), the kernel matrix never formed (stpy_kmv_dxx in the header; SE and Matern 5/2, d <= 16).  Vt: (t, |b|), may be a
	column window of wider storage; out: (t, |a|, >= 1 + d + d (d + 1) / 2) with a unit last stride, may be a window of wider storage in both
	leading dimensions."""
	n, q, d, t = a.shape[0], b.shape[0], _ncols(a, cols), Vt.shape[0]
	nc = kmv_dxx_ncol(d)
	if out.dim() != 3 or out.shape[0] != t or out.shape[1] != n or out.shape[2] < nc or out.stride(2) != 1:
		raise StpyHipError("kmv_dxx: out must be (t, n, >= 1 + d + d (d + 1) / 2) = (%d, %d, >= %d) with a unit last stride, got %s" % (t, n, nc, tuple(out.shape)))
	ldo = out.stride(1) if n > 1 else max(out.stride(1), int(out.shape[2]))
	ldc = out.stride(0) if t > 1 else max(out.stride(0), n * ldo)
	work = kmv_dxx_workspace(n, q, d, t, out) if work is None else work
	_launch("stpy_kmv_dxx", kind, dtype_code(out.dtype), ptr(a), n, ld(a), ptr(b), q, ld(b), d, ptr(cols), ptr(inv_ls), float(kappa),
			ptr(Vt), ld(Vt), t, ptr(out), ldc, ldo, ptr(work), work.numel())


def rff_embed(x, W, m, scale, bias=None, feat_scale=None, transposed=False, workspace=False):
	"""Random-feature embedding of the rows of x by the first m rows of W: (n, m), or (m, n) when ``transposed``.  ``workspace``
	passes the library's, which moves the large fp32 d = 64 shapes to the bf16 matrix cores."""
	n, d = x.shape
	out = torch.empty((m, n) if transposed else (n, m), dtype=x.dtype, device=x.device)
	wb = int(load().stpy_rff_workspace_bytes(dtype_code(x.dtype), n, d, m)) if workspace else 0
	work = _work(wb, x) if wb > 0 else None
	_launch("stpy_rff_embed", dtype_code(x.dtype), ptr(x), n, ld(x), d, ptr(W), ld(W), m, ptr(bias), ptr(feat_scale), scale, ptr(out), ld(out),
			int(transposed), ptr(work), wb)
	return out


def rff_grad(x, W, m, scale, C, G, bias=None, feat_scale=None, val=None, H=None, combine=OUT_SET):
	"""G[t] (combine)= d/dx_t sum_j C[t, j] phi_j(x_t) for the feature map of rff_embed (same W, m, scale, bias, feat_scale);
	``val`` (n,) also receives the sums themselves and ``H`` (n, ld(G), ld(G)) their Hessians.  C: (n, m) rows, may be a column
	window of a wider matrix, or ONE row (a 1-D tensor of m elements) shared by all points."""
	n, d = x.shape
	order = 1 if H is None else 2
	ldc = 0 if C.dim() == 1 else ld(C)
	work = _work(max(int(load().stpy_rff_grad_workspace_bytes(dtype_code(x.dtype), n, d, m, order)), 1), x)
	_launch("stpy_rff_grad", dtype_code(x.dtype), ptr(x), n, ld(x), d, ptr(W), ld(W), m, ptr(bias), ptr(feat_scale), float(scale), ptr(C), ldc,
			order, combine, ptr(val), ptr(G), ld(G), ptr(H), ptr(work), work.numel())
