"""
tests/bc_cases.py pinned on the CPU: the enumeration-based block-cyclic oracle the GPU staircase tests (tests/test_gpu_gemm_bc.py)
stand on, and through it the CPU stand-in ``CpuLocalOps.gemm_nt(bc=...)`` the gloo block-cyclic tests run on.
"""
import pytest
import torch

from tests import bc_cases as bc
from tests.cpu_local_ops import CpuLocalOps

# (N, NB, pr, pc): aligned and ragged N (ragged inside a tile too), every grid shape the GPU tests use
GRIDS = [(640, 128, 1, 1), (1280, 256, 1, 2), (1100, 256, 1, 2), (1536, 128, 2, 2), (1500, 256, 2, 4), (1408, 128, 4, 2), (2560, 512, 2, 4), (1900, 512, 2, 2)]


@pytest.mark.parametrize("N,NB,pr,pc", GRIDS)
def test_gather_inverts_scatter(N, NB, pr, pc):
	G = torch.arange(N * N, dtype=torch.float64).reshape(N, N)
	loc = bc.scatter(G, NB, pr, pc)
	assert sum(l.numel() for l in loc.values()) == N * N
	# every rank's rows and columns are whole global blocks, in increasing global order
	for (r, c), l in loc.items():
		assert torch.equal(l[:, 0] // N, torch.tensor(bc.owned_index(N, NB, pr, r), dtype=torch.float64))
		assert torch.equal(l[0, :] % N, torch.tensor(bc.owned_index(N, NB, pc, c), dtype=torch.float64))
	assert torch.equal(bc.gather(loc, N, NB, pr, pc), G)


@pytest.mark.parametrize("form", ["split", "single"])
@pytest.mark.parametrize("N,NB,pr,pc", GRIDS)
def test_needed_mask_is_the_scattered_global_lower_triangle(N, NB, pr, pc, form):
	"""for every rank, step and call: needed_mask == the window's tiles of the scattered global lower-tile indicator; and the windows of one
	step together cover exactly the trailing matrix's lower tiles"""
	nblk = (N + NB - 1) // NB
	low = bc.lower_tiles(N)
	low_loc = bc.scatter(low, NB, pr, pc)
	for K in range(nblk - 1):
		seen = {rc: torch.zeros_like(l, dtype=torch.int32) for rc, l in low_loc.items()}
		for r in range(pr):
			for c in range(pc):
				i0, calls = bc.rank_window(nblk, NB, pr, pc, r, c, K, form)
				for j0, j1 in calls:
					win = low_loc[(r, c)][i0 * NB:, j0 * NB:j1 * NB]
					m, n = win.shape
					if m == 0:
						continue
					mask = bc.needed_mask(m, n, NB, pr, pc, r, c, i0, j0)
					assert torch.equal(bc.expand_tiles(mask, m, n), win), (K, r, c, j0)
					assert torch.equal(mask, win[::bc.TILE, ::bc.TILE])
					seen[(r, c)][i0 * NB:, j0 * NB:j1 * NB] += 1
		s = (K + 1) * NB
		want = torch.zeros(N, N, dtype=torch.int32)
		want[s:, s:] = 1
		assert torch.equal(bc.gather(seen, N, NB, pr, pc) * low, want * low), K          # each trailing lower tile lies in exactly one window


@pytest.mark.parametrize("form", ["split", "single"])
@pytest.mark.parametrize("N,NB,pr,pc,k", [(640, 128, 1, 1, 8), (1100, 256, 1, 2, 24), (1536, 128, 2, 2, 8), (1500, 256, 2, 4, 16), (1408, 128, 4, 2, 8), (2560, 512, 2, 4, 8)])
def test_cpu_local_ops_staircase_against_the_global_oracle(N, NB, pr, pc, k, form):
	"""CpuLocalOps.gemm_nt(bc=...) through a whole right-looking sweep: the gathered result is the global lower-tile update, entry by entry
	within the fma bound; tiles above the global tile diagonal keep their bits"""
	ops = CpuLocalOps()
	g = torch.Generator().manual_seed(N + NB + 7 * pr + pc)
	nblk = (N + NB - 1) // NB
	C0 = torch.randn(N, N, dtype=torch.float64, generator=g)
	panels = [torch.randn(N, k, dtype=torch.float64, generator=g) for _ in range(nblk - 1)]
	got = bc.sweep(lambda A, B, C, w: ops.gemm_nt(A, B, C, 1, bc=w), C0, panels, NB, pr, pc, form)
	ref, bracket, low = bc.sweep_reference(C0, panels, NB)
	assert torch.equal(got[~low], C0[~low])
	ratio = bc.worst_ratio(got, ref, bracket, nblk - 1, k, torch.float64)
	print("cpu stand-in %dx%d N=%d NB=%d %s: worst error / bound %.3g" % (pr, pc, N, NB, form, ratio))
	assert ratio <= 1.0


def test_cpu_local_ops_single_window_modes():
	"""one window the staircase crosses, mode 0 and mode 1: needed tiles written, the others (NaN) neither read nor written"""
	ops = CpuLocalOps()
	m, n, k, w = 1152, 896, 16, (256, 2, 4, 0, 2, 1, 0)
	g = torch.Generator().manual_seed(5)
	A, B = torch.randn(m, k, dtype=torch.float64, generator=g), torch.randn(n, k, dtype=torch.float64, generator=g)
	need = bc.expand_tiles(bc.needed_mask(m, n, *w), m, n)
	assert need.any() and not need.all()
	for mode in (0, 1):
		C0 = torch.randn(m, n, dtype=torch.float64, generator=g)
		C = torch.where(need, C0, torch.full_like(C0, float("nan")))
		ops.gemm_nt(A, B, C, mode, bc=w)
		want = A @ B.T if mode == 0 else C0 - A @ B.T
		assert torch.isnan(C[~need]).all()
		assert bc.worst_ratio(C[need], want[need], (C0.abs() + A.abs() @ B.abs().T)[need], 1, k, torch.float64) <= 1.0
