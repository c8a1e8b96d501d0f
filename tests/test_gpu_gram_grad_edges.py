"""
stpy_gram_grad (csrc/grad.hip) through the C ABI on the cases of tests/gram_grad_cases.py, which has the inputs, the longdouble oracle and the
derived entrywise bound (tests/test_gram_grad_cases_cpu.py shows on the CPU that they separate a right evaluation from a wrong one).  Both
dtypes, all six families, gradient and Hessian.

What is pinned, and by what:
  values       |G - G_true| and |H - H_true| entry by entry within c eps S, S the sum of the absolute values of the entry's terms -- on
               centred, off-centre, duplicate, clustered and extreme-lengthscale points, at every boundary of grad_plan and of the kernel's
               tiles, for every coefficient form (alpha / u / Wt / v with their NULLs, ldw > n), through a non-monotone column subset with
               ldt != ldx and ldg > d, under SET and ADD;
  translation  the SAME BITS on a layout's integer translate (its twin): the coordinates are subtracted before they are scaled;
  determinism  the same bits when the same call runs twice;
  ownership    every entry of G and H outside cols, and past column d, keeps the bits it started with (a sentinel, or random contents);
  finiteness   no NaN or Inf on the tiny- and huge-lengthscale layouts (nor anywhere else: the bound fails on one);
  exactness    a coincident single pair gives G exactly 0 and an exactly diagonal H with c psi(0) inv_ls_k^2 on it, to the bound.
Each test prints its largest error / bound per group of cases on a line tagged GRADEDGE (`-s` shows them; DESIGN.md tabulates them).
"""
import numpy as np
import pytest
import torch

from tests import gram_edge_cases as E
from tests import gram_grad_cases as C

pytestmark = pytest.mark.gpu

TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
DTS = ["f64", "f32"]


@pytest.fixture(scope="module")
def L(gpu_device):
	from stpy_amd import _lib
	return _lib


@pytest.fixture(autouse=True)
def _drop_cached_cases():
	yield
	E.make_case.cache_clear()


def dev(a, dt):
	return None if a is None else torch.from_numpy(np.array(a, order="C")).to(device="cuda:0", dtype=TORCH_DT[dt])


def run(L, gc, runs=1):
	"""The call of the case, `runs` times from the same initial G and H; returns [(Gbuf, Hbuf)] as numpy arrays of the dtype."""
	lib, dt = L.load(), gc.dt
	code = L.dtype_code(TORCH_DT[dt])
	x, xt, il = dev(gc.x, dt), dev(gc.xt, dt), dev(gc.inv_ls, dt)
	alpha, u, Wt, v = dev(gc.alpha, dt), dev(gc.u, dt), dev(gc.Wt, dt), dev(gc.v, dt)
	cols = torch.tensor(gc.cols, dtype=torch.int32, device="cuda:0") if gc.cols is not None else None
	nbytes = int(lib.stpy_gram_grad_workspace_bytes(code, gc.m, gc.n, gc.d, gc.order))
	Q, _, _, nsplit, _ = C.plan(gc.m, gc.n, gc.d, gc.order)
	assert nbytes == nsplit * gc.m * Q * (8 if dt == "f64" else 4), "plan() of the cases and grad_plan of the kernel disagree"
	out = []
	for _ in range(runs):
		G, H = dev(gc.G0, dt), dev(gc.H0, dt)
		work = torch.full((nbytes,), 0xff, dtype=torch.uint8, device="cuda:0")          # (NaN patterns: a partial sum read unwritten shows)
		L.check(lib.stpy_gram_grad(gc.kind | (gc.degree << 8), code, L.ptr(x), gc.n, gc.x.shape[1], L.ptr(xt), gc.m, gc.xt.shape[1], gc.d, L.ptr(cols),
		                           L.ptr(il), gc.kappa, gc.offset, L.ptr(alpha), L.ptr(u), L.ptr(Wt), gc.Wt.shape[1] if gc.Wt is not None else 0, L.ptr(v),
		                           gc.order, gc.combine, L.ptr(G), gc.ldg, L.ptr(H), L.ptr(work), nbytes, L.stream_ptr()), "stpy_gram_grad")
		torch.cuda.synchronize()
		out.append((G.cpu().numpy(), None if H is None else H.cpu().numpy()))
	return out


def same_bits(a, b):
	return np.array_equal(a[0], b[0], equal_nan=True) and (a[1] is None or np.array_equal(a[1], b[1], equal_nan=True))


def group_of(gc):
	return gc.name.split("-")[0]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_every_case_of_a_family(L, family, dt):
	"""All cases of gram_grad_cases.cases(dt, family); every violation is collected, so one run shows them all."""
	cs = C.cases(dt, family)
	got, worst, failures = {}, {}, []
	for gc in cs:
		first, second = run(L, gc, runs=2)
		got[gc.name] = first
		if not same_bits(first, second):
			failures.append("%s: two runs of the same call differ" % gc.name)
		r = C.check(gc, *first)
		g = group_of(gc)
		worst[g] = max(worst.get(g, (0.0, 0.0, 0.0)), (r["ratio"], r["ratio_G"], r["ratio_H"]))
		if not r["ratio"] <= 1.0:
			failures.append("%s: error / bound %.3g (G %.3g, H %.3g)" % (gc.name, r["ratio"], r["ratio_G"], r["ratio_H"]))
		if not r["untouched"]:
			failures.append("%s: entries outside cols / past column d were written" % gc.name)
		if g in ("tiny_lengthscale", "huge_lengthscale"):
			owned = C.gather(gc, *first)
			if not all(np.all(np.isfinite(o)) for o in owned if o is not None):
				failures.append("%s: NaN or Inf" % gc.name)
		if gc.twin_of is not None and not same_bits(first, got[gc.twin_of]):
			dG = float(np.max(np.abs(first[0].astype(np.float64) - got[gc.twin_of][0].astype(np.float64)) / (gc.eps * np.maximum(C.oracle(gc)["S_G"].astype(np.float64), gc.tiny))))
			failures.append("%s: the twin does not have the bits of %s (G differs by up to %.3g eps S)" % (gc.name, gc.twin_of, dG))
		if g == "exact":
			if not (r["exact_zero_G"] and r.get("exact_zero_offdiag_H", True)):
				failures.append("%s: a coincident pair must give G == 0 and an exactly diagonal H" % gc.name)
	for g in sorted(worst):
		print("GRADEDGE %-7s %s %-30s largest error / bound %.3g  (G %.3g, H %.3g)" % ((family, dt, g) + worst[g]))
	print("GRADEDGE %-7s %s all %d cases: worst error / bound %.3g" % (family, dt, len(cs), max(w[0] for w in worst.values())))
	assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dt", DTS)
def test_exact_hessian_of_a_coincident_pair(L, dt):
	"""n = m = 1, xt == x: H is c (-kappa) inv_ls_k^2 on the diagonal for SE and c (-(5 / 3) kappa) inv_ls_k^2 for Matern 5/2, to the bound; G and
	the off-diagonal of H are exactly 0; Matern 1/2 and 3/2 give G exactly 0."""
	for family, psi0 in (("se", -1.0), ("m52", -5.0 / 3.0), ("m12", None), ("m32", None)):
		gc, = C.exact_cases(dt, family)
		(G, H), = run(L, gc)
		assert np.all(G == 0), (family, G)
		if psi0 is not None:
			o = C.oracle(gc)
			c = gc.u[0] * gc.alpha[0]
			want = c * psi0 * gc.kappa * gc.inv_ls ** 2
			err = np.abs(np.diag(H[0]).astype(np.float64) - want)
			bound = np.diag(o["bH"][0]).astype(np.float64) + 4 * np.finfo(np.float64).eps * np.abs(want)
			print("GRADEDGE %-7s %s coincident pair: H diagonal error / bound %.3g" % (family, dt, float(np.max(err / bound))))
			assert np.all(err <= bound), (family, err / bound)
			assert np.all(H[0][~np.eye(gc.d, dtype=bool)] == 0), (family, H)
