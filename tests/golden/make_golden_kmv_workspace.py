"""
Writes tests/golden/W1_kmv_workspace.json: what the five workspace queries of the matrix-free family (stpy_kmv, stpy_pcg, stpy_kmv_dtheta,
stpy_kmv_dx, stpy_kmv_dxx) return over a grid of arguments, recorded from the built library on the CPU (the queries touch no device).
tests/test_kmv_workspace_cpu.py asks the library again and compares, so the file pins the split policy wherever a query exposes it:
exactly for stpy_kmv_dx and stpy_kmv_dtheta (they report the size of the cut they make), as an envelope for the others.

The grid: n over SIZES, q over 0 and SIZES, t over TS, d over DS, both types, and for stpy_pcg r over RS.  Per query, type and d the values
are walked in the order (t, n, q) -- the arguments a query does not take are left out of its walk -- and stored as runs [bytes, count].
stpy_kmv's and stpy_pcg's queries do not look at d: their walks are the same for every d, are checked to be, and are stored once (key without
a d); the test still asks for every d.

The committed file was recorded from the library as built at the commit before csrc/kmv_pair.h existed (four separate split functions).
Regenerate only when a change to a workspace size is intended, from the repository root:

    python tests/golden/make_golden_kmv_workspace.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
	sys.path.insert(0, ROOT)

PATH = os.path.join(ROOT, "tests", "golden", "W1_kmv_workspace.json")
SIZES = (1, 2, 5, 63, 64, 65, 256, 257, 1000, 4099, 16320, 16321, 65536, 1 << 20, (1 << 31) - 1)
QS = (0,) + SIZES
TS = (1, 2, 15, 16, 17, 63, 64, 65, 70, 1000, 1 << 16)
DS = (1, 3, 8, 16, 17, 40)
RS = (0, 1, 64)


def walks(lib):
	"""{name: the query's values in walk order}, one entry per (query, dtype, d) and, for stpy_pcg, r."""
	out = {}
	for dtype in (0, 1):
		for d in DS:
			key = "f%d/d%d" % (32 if dtype else 64, d)
			out["stpy_kmv/" + key] = [lib.stpy_kmv_workspace_bytes(dtype, n, q, d, t) for t in TS for n in SIZES for q in QS]
			out["stpy_kmv_dx/" + key] = [lib.stpy_kmv_dx_workspace_bytes(dtype, n, q, d, t) for t in TS for n in SIZES for q in QS]
			out["stpy_kmv_dxx/" + key] = [lib.stpy_kmv_dxx_workspace_bytes(dtype, n, q, d, t) for t in TS for n in SIZES for q in QS]
			out["stpy_kmv_dtheta/" + key] = [lib.stpy_kmv_dtheta_workspace_bytes(dtype, n, d, t) for t in TS for n in SIZES]
			for r in RS:
				out["stpy_pcg/%s/r%d" % (key, r)] = [lib.stpy_pcg_workspace_bytes(dtype, n, d, t, r) for t in TS for n in SIZES]
	return out


def runs(values):
	out = []
	for v in values:
		if out and out[-1][0] == v:
			out[-1][1] += 1
		else:
			out.append([v, 1])
	return out


def stored_key(name):
	"""The fixture's key of a walk: without the d of a query that ignores it."""
	parts = name.split("/")
	return "/".join(p for p in parts if not (parts[0] in ("stpy_kmv", "stpy_pcg") and p[0] == "d"))


def main():
	from stpy_amd import _lib
	stored = {}
	for name, v in walks(_lib.load()).items():
		assert stored.setdefault(stored_key(name), v) == v, name
	lines = ['"%s": %s' % (name, json.dumps(runs(v), separators=(",", ":"))) for name, v in stored.items()]
	with open(PATH, "w") as fh:
		fh.write("{\n" + ",\n".join(lines) + "\n}\n")
	print("wrote %s: %d walks, %d bytes" % (PATH, len(lines), os.path.getsize(PATH)))


if __name__ == "__main__":
	main()
