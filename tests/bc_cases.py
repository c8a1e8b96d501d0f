"""
The 2-D block-cyclic distribution stated in GLOBAL terms, by enumeration -- TEST INFRASTRUCTURE ONLY.

``stpy_gemm_nt_bc`` decides from (nb_dist, pr, pc, myr, myc, i0, j0) which 128 x 128 tiles of a rank's local window it updates.
Nothing here repeats that index arithmetic.  The distribution is written down once, as lists:

  * global block I (NB rows, the last one possibly shorter) belongs to process row I % pr;
  * a rank's local row blocks are its global blocks in increasing order; columns likewise with pc;

and everything else -- which global rows a rank holds, where a window starts after panel step K, which tiles of a window lie on or
below the global tile diagonal -- is looked up in those lists.  The expectation of every test built on this file is "the lower
128-tile triangle of the GLOBAL matrix".

No GPU import at module level; the tensors may live on any device.
"""
import math

import torch

TILE = 128


def owned_blocks(nblk, p, r):
	"""global block indices of process row (or column) r of p, in local order"""
	return [I for I in range(nblk) if I % p == r]


def owned_index(N, NB, p, r):
	"""global row (or column) indices held by process row (or column) r of p, in local order"""
	idx = []
	for I in owned_blocks((N + NB - 1) // NB, p, r):
		idx.extend(range(I * NB, min(N, I * NB + NB)))
	return idx


def _index(idx, like):
	return torch.as_tensor(idx, dtype=torch.long, device=like.device)


def scatter(G, NB, pr, pc):
	"""global matrix -> {(r, c): local matrix} (copies)"""
	N, M = G.shape
	rows = [_index(owned_index(N, NB, pr, r), G) for r in range(pr)]
	cols = [_index(owned_index(M, NB, pc, c), G) for c in range(pc)]
	return {(r, c): G[rows[r]][:, cols[c]].contiguous() for r in range(pr) for c in range(pc)}


def gather(loc, N, NB, pr, pc, M=None):
	"""inverse of scatter"""
	M = N if M is None else M
	any_loc = loc[(0, 0)]
	G = torch.empty((N, M), dtype=any_loc.dtype, device=any_loc.device)
	for c in range(pc):
		ci = _index(owned_index(M, NB, pc, c), any_loc)
		strip = torch.empty((N, ci.numel()), dtype=any_loc.dtype, device=any_loc.device)
		for r in range(pr):
			strip[_index(owned_index(N, NB, pr, r), any_loc)] = loc[(r, c)]
		G[:, ci] = strip
	return G


def rank_window(nblk, NB, pr, pc, r, c, K, form="split"):
	"""Where rank (r, c) updates after panel step K: (i0, [(j0, j1), ...]) in LOCAL block indices, one entry per call.  The window
	of a call is rows i0 * NB .. end and columns j0 * NB .. j1 * NB of the local matrix.
	form "split":  block column K+1 alone if this rank holds it, then its columns beyond K+1 (the factorisation's look-ahead order);
	form "single": all its columns beyond K in one call."""
	rows, cols = owned_blocks(nblk, pr, r), owned_blocks(nblk, pc, c)
	i0 = sum(1 for I in rows if I <= K)
	calls = []
	if form == "split":
		if K + 1 in cols:
			jc = cols.index(K + 1)
			calls.append((jc, jc + 1))
		j1 = sum(1 for J in cols if J <= K + 1)
		if j1 < len(cols):
			calls.append((j1, len(cols)))
	else:
		j0 = sum(1 for J in cols if J <= K)
		if j0 < len(cols):
			calls.append((j0, len(cols)))
	return i0, calls


def _nth_owned(p, r, b):
	"""global index of local block b of process row (or column) r of p"""
	return owned_blocks((b + 1) * p, p, r)[b]


def needed_mask(m, n, nb_dist, pr, pc, myr, myc, i0, j0):
	"""bool (tiles_m, tiles_n): tile (ti, tj) of the m x n window at local block (i0, j0) lies on or below the GLOBAL tile diagonal"""
	nbt = nb_dist // TILE
	tm, tn = (m + TILE - 1) // TILE, (n + TILE - 1) // TILE
	grow = [_nth_owned(pr, myr, i0 + ti // nbt) * nbt + ti % nbt for ti in range(tm)]
	gcol = [_nth_owned(pc, myc, j0 + tj // nbt) * nbt + tj % nbt for tj in range(tn)]
	return torch.tensor([[gr >= gc for gc in gcol] for gr in grow], dtype=torch.bool).reshape(tm, tn)


def expand_tiles(mask, m, n, device=None):
	"""tile mask -> element mask of an m x n window"""
	if device is not None:
		mask = mask.to(device)
	return mask.repeat_interleave(TILE, 0)[:m].repeat_interleave(TILE, 1)[:, :n]


def lower_tiles(N, device=None):
	"""element mask of the lower 128-tile triangle of an N x N matrix"""
	nt = (N + TILE - 1) // TILE
	return expand_tiles(torch.ones(nt, nt, dtype=torch.bool).tril(), N, N, device)


def sweep(call, C0, panels, NB, pr, pc, form):
	"""The trailing updates of a right-looking factorisation of the N x N matrix C0 with the given panels (panels[K]: N x k, applied
	after step K to everything beyond block K), every rank of the pr x pc grid played in turn through
	``call(A, B, Cwindow, (nb_dist, pr, pc, myr, myc, i0, j0))`` in mode 1.  Returns the gathered result."""
	N = C0.shape[0]
	nblk = (N + NB - 1) // NB
	loc = scatter(C0, NB, pr, pc)
	rows = [_index(owned_index(N, NB, pr, r), C0) for r in range(pr)]
	cols = [_index(owned_index(N, NB, pc, c), C0) for c in range(pc)]
	for K in range(nblk - 1):
		P = panels[K]
		prow = [P[rows[r]] for r in range(pr)]
		pcol = [P[cols[c]] for c in range(pc)]
		for r in range(pr):
			for c in range(pc):
				i0, calls = rank_window(nblk, NB, pr, pc, r, c, K, form)
				A = prow[r][i0 * NB:]
				if A.shape[0] == 0:
					continue
				for j0, j1 in calls:
					call(A, pcol[c][j0 * NB:j1 * NB], loc[(r, c)][i0 * NB:, j0 * NB:j1 * NB], (NB, pr, pc, r, c, i0, j0))
	return gather(loc, N, NB, pr, pc)


def sweep_reference(C0, panels, NB):
	"""(ref, bracket) in fp64: ref = C0 - sum_K lowtiles(P_K[s:] P_K[s:]^T), s = (K+1) NB; bracket = |C0| + sum_K |P_K[s:]| |P_K[s:]|^T,
	the quantity the entry-wise error bound multiplies"""
	N = C0.shape[0]
	nblk = (N + NB - 1) // NB
	Q = torch.cat([panels[K].double() for K in range(nblk - 1)], dim=1)
	k = panels[0].shape[1]
	for K in range(nblk - 1):
		Q[:(K + 1) * NB, K * k:(K + 1) * k] = 0
	low = lower_tiles(N, C0.device)
	ref = C0.double() - torch.where(low, Q @ Q.T, torch.zeros((), dtype=torch.float64, device=C0.device))
	Q.abs_()
	bracket = C0.double().abs() + Q @ Q.T
	return ref, bracket, low


def gamma(nterms, dtype):
	"""gamma_n = n u / (1 - n u): the relative bound of an n-term sum of products accumulated by fused multiply-adds in any order"""
	u = 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24
	return nterms * u / (1.0 - nterms * u)


def worst_ratio(got, ref, bracket, nupdates, k, dtype):
	"""max over entries of |got - ref| / (f gamma_{S (k+1)} bracket); f = 2 when the fp64 reference carries the same error as
	the result (fp64 against fp64), 1 for fp32 against the fp64 reference.  NaN (a non-finite result) counts as infinite."""
	f = 2.0 if dtype == torch.float64 else 1.0
	bound = bracket * (f * gamma(nupdates * (k + 1), dtype))
	ratio = (got.double() - ref).abs_() / bound
	ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
	return float(ratio.max())
