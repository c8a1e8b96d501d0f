"""In-process A/B of two builds of the library (tools/_ab/libstpy_hip_base.so = a baseline build, stpy_amd/libstpy_hip.so =
the tree): the trailing-update GEMM at a few shapes, then the whole fit + mean_std step through the C ABI calls the
estimator makes; the step's factor and solve must come out byte-equal.
  potrf      stpy_potrf alone: lower triangle, winv and info byte for byte at the smallest orders that reach each branch of the
             driver (fp64 and fp32, flags 0 and STPY_FLAG_BESIDE_UPDATE, one failing pivot), then its time with the builds
             alternating in one process.  With a second baseline build (tools/_ab/libstpy_hip_base2.so, same sources as the first)
             the per-round range of base / base2 is the margin the tree / base ratio is read against.
  step [n,..] only the whole step, at these orders
usage: python tools/ab_libs.py [potrf | step [n,..]]"""
import ctypes, os, sys, time, math
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stpy_amd import _lib as L

def bind(path):
	lib = ctypes.CDLL(path)
	for name, (res, args) in L.SIGNATURES.items():
		if hasattr(lib, name):
			fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
	return lib

libs = {"base": bind(os.path.join(ROOT, "tools", "_ab", "libstpy_hip_base.so")), "tree": bind(os.path.join(ROOT, "stpy_amd", "libstpy_hip.so"))}
base2 = os.path.join(ROOT, "tools", "_ab", "libstpy_hip_base2.so")
if os.path.exists(base2):
	libs["base2"] = bind(base2)
dev = torch.device("cuda:0")
mode = sys.argv[1] if len(sys.argv) > 1 else ""

def timeit(f, reps=3):
	ts = []
	for _ in range(reps):
		torch.cuda.synchronize(); t0 = time.perf_counter(); f(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
	return min(ts)

def lower_equal(A, B, rows=4096):          # byte equality of the lower triangles (what lies above is scratch by contract)
	return all(torch.equal(torch.tril(A[i:i + rows], diagonal=i), torch.tril(B[i:i + rows], diagonal=i)) for i in range(0, A.shape[0], rows))

def potrf_once(lib, K, nb, flags):
	dt, n = K.dtype, K.shape[0]
	code = L.dtype_code(dt)
	A = K.clone()
	winv = torch.zeros(int(lib.stpy_potrf_winv_elems(n)), dtype=dt, device=dev)
	work = torch.empty(int(lib.stpy_potrf_workspace_bytes(code, n, nb)), dtype=torch.uint8, device=dev)
	info = torch.zeros(1, dtype=torch.int32, device=dev)
	assert lib.stpy_potrf(code, n, L.ptr(A), n, L.ptr(winv), winv.numel(), L.ptr(work), work.numel(), nb, flags, L.ptr(info), L.stream_ptr()) == 0
	torch.cuda.synchronize()
	return A, winv, int(info.item())

def spd(n, dt, seed):
	g = torch.Generator(device=dev); g.manual_seed(seed)
	G = torch.randn(n, 64, dtype=torch.float64, device=dev, generator=g)
	K = G @ G.T
	K.diagonal().add_(64.0)
	return K.to(dt)

def potrf_bits():
	bad = 0
	for dt in (torch.float64, torch.float32):
		for n, nb in ((128, 0), (1000, 256), (2048, 512), (4096, 0), (8192, 0)):
			K = spd(n, dt, n)
			for flags in (0, L.FLAG_BESIDE_UPDATE):
				A0, W0, i0 = potrf_once(libs["base"], K, nb, flags)
				A1, W1, i1 = potrf_once(libs["tree"], K, nb, flags)
				ok = lower_equal(A0, A1) and torch.equal(W0, W1) and i0 == i1 == 0
				bad += not ok
				print("potrf bits %s n=%d nb=%d flags=%d: L %s  winv %s  info %d / %d" % (str(dt).split(".")[1], n, nb, flags, lower_equal(A0, A1), torch.equal(W0, W1), i0, i1), flush=True)
	K = spd(1536, torch.float64, 1536)
	K[1100, 1100] = -1.0
	infos = [potrf_once(libs[nm], K, 256, 0)[2] for nm in ("base", "tree")]
	print("potrf failing pivot n=1536 nb=256 K[1100,1100]=-1: info %d / %d" % tuple(infos), flush=True)
	bad += infos != [1101, 1101]
	return bad

def potrf_times(rounds=9):
	for n, dt in ((8192, torch.float64), (16384, torch.float64), (16384, torch.float32)):
		code = L.dtype_code(dt)
		K0 = spd(n, dt, n)
		K = torch.empty_like(K0)
		winv = torch.zeros(int(libs["tree"].stpy_potrf_winv_elems(n)), dtype=dt, device=dev)
		work = torch.empty(int(libs["tree"].stpy_potrf_workspace_bytes(code, n, 0)), dtype=torch.uint8, device=dev)
		info = torch.zeros(1, dtype=torch.int32, device=dev)
		ts = {nm: [] for nm in libs}
		for rnd in range(rounds + 1):          # (round 0 warms every build up)
			for nm, lib in libs.items():
				K.copy_(K0)
				e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
				torch.cuda.synchronize()
				e0.record()
				assert lib.stpy_potrf(code, n, L.ptr(K), n, L.ptr(winv), winv.numel(), L.ptr(work), work.numel(), 0, 0, L.ptr(info), L.stream_ptr()) == 0
				e1.record()
				torch.cuda.synchronize()
				if rnd > 0:
					ts[nm].append(e0.elapsed_time(e1))
		line = "potrf time %s n=%d: " % (str(dt).split(".")[1], n) + "  ".join("%s median %.3f min %.3f ms" % (nm, np.median(v), min(v)) for nm, v in ts.items())
		r = np.array(ts["tree"]) / np.array(ts["base"])
		line += "   tree/base per round: median %.4f [%.4f, %.4f]" % (np.median(r), r.min(), r.max())
		if "base2" in ts:
			pp = np.array(ts["base2"]) / np.array(ts["base"])
			line += "   base2/base: median %.4f [%.4f, %.4f]  -> tree %s the margin" % (np.median(pp), pp.min(), pp.max(), "INSIDE" if pp.min() <= np.median(r) <= pp.max() else "OUTSIDE")
		print(line, flush=True)
		del K0, K, winv, work

if mode == "potrf":
	bad = potrf_bits()
	potrf_times()
	sys.exit("ab_libs: %d potrf case(s) differ between the builds" % bad if bad else 0)

for n, k in ((32768, 1024), (32768, 256), (16384, 512)) if mode == "" else ():
	P = torch.randn(n, k, dtype=torch.float64, device=dev)
	C = torch.randn(n, n, dtype=torch.float64, device=dev)
	res = {}
	for rnd in range(3):
		for name, lib in libs.items():
			f = lambda: lib.stpy_gemm_nt(L.F64, n, n, k, L.ptr(P), k, L.ptr(P), k, L.ptr(C), n, 1, 1, L.stream_ptr())
			f(); res.setdefault(name, []).append(timeit(f))
	fl = 2.0 * n * n * k * (0.5 + 64.0 / n)
	print("syrk n=%d k=%d: " % (n, k) + "  ".join("%s %.3f ms %.2f TF" % (nm, min(v) * 1e3, fl / min(v) / 1e12) for nm, v in res.items()), flush=True)
	del P, C

def step(lib, n, d, m, x, xt, y):
	code = L.F64
	il = torch.full((d,), 1.0 / math.sqrt(d), dtype=torch.float64, device=dev)
	K = torch.empty(n, n, dtype=torch.float64, device=dev)
	ws = torch.empty(int(lib.stpy_gram_workspace_bytes(code, n, n, d)), dtype=torch.uint8, device=dev)
	winv = torch.empty(int(lib.stpy_potrf_winv_elems(n)), dtype=torch.float64, device=dev)
	work = torch.empty(int(lib.stpy_potrf_workspace_bytes(code, n, 0)), dtype=torch.uint8, device=dev)
	info = torch.zeros(1, dtype=torch.int32, device=dev)
	X = torch.empty(m, n, dtype=torch.float64, device=dev)
	ws2 = torch.empty(int(lib.stpy_gram_workspace_bytes(code, n, m, d)), dtype=torch.uint8, device=dev)
	tw = torch.empty(int(lib.stpy_trsm_workspace_bytes(code, m, n, 0)), dtype=torch.uint8, device=dev)
	def run():
		assert lib.stpy_gram(0, code, L.ptr(x), n, d, L.ptr(x), n, d, d, None, L.ptr(il), 1.0, 0.0, 0.01, 1, 0, L.ptr(K), n, L.ptr(ws), ws.numel(), L.stream_ptr()) == 0
		assert lib.stpy_potrf(code, n, L.ptr(K), n, L.ptr(winv), winv.numel(), L.ptr(work), work.numel(), 0, 0, L.ptr(info), L.stream_ptr()) == 0
		assert lib.stpy_gram(0, code, L.ptr(x), n, d, L.ptr(xt), m, d, d, None, L.ptr(il), 1.0, 0.0, 0.0, 0, 0, L.ptr(X), n, L.ptr(ws2), ws2.numel(), L.stream_ptr()) == 0
		assert lib.stpy_trsm_right_lt(code, m, n, L.ptr(K), n, L.ptr(winv), winv.numel(), L.ptr(X), n, 0, 0, L.ptr(tw) if tw.numel() else None, tw.numel(), L.stream_ptr()) == 0
	return run, (K, X)

sizes = [(int(v), 8 if int(v) <= 16384 else 16, 4096) for v in sys.argv[2].split(",")] if mode == "step" and len(sys.argv) > 2 else [(16384, 8, 4096), (65536, 16, 4096)]
differ = 0
for n, d, m in sizes:
	x = torch.rand(n, d, dtype=torch.float64, device=dev) * 2 - 1
	xt = torch.rand(m, d, dtype=torch.float64, device=dev) * 2 - 1
	res, chk, outs = {}, {}, {}
	for name in ("base", "tree"):
		lib = libs[name]
		run, (K, X) = step(lib, n, d, m, x, xt, None)
		run(); torch.cuda.synchronize()
		for rnd in range(3):
			res.setdefault(name, []).append(timeit(run, reps=1))
		chk[name] = (float(X[:, ::7].norm()), float(K.diagonal().sum()))
		outs[name] = (K, X)
		del run
	same = lower_equal(outs["base"][0], outs["tree"][0]) and torch.equal(outs["base"][1], outs["tree"][1])
	differ += not same
	print("gram+potrf+K*+trsm n=%d m=%d: " % (n, m) + "  ".join("%s %.4f s" % (nm, min(v)) for nm, v in res.items()) + "   |X| %r  |L| %r   factor and solve byte-equal: %s" % (chk["base"], chk["tree"], same), flush=True)
	del outs
	torch.cuda.empty_cache()
if differ:
	sys.exit("ab_libs: the step differs between the builds at %d size(s)" % differ)
