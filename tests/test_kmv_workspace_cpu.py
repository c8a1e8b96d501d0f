"""
The workspace queries of the matrix-free family return what tests/golden/W1_kmv_workspace.json recorded, argument for argument: the split
policy (csrc/kmv_pair.h) is pinned wherever a query exposes it -- exactly for stpy_kmv_dx and stpy_kmv_dtheta, as an envelope for stpy_kmv,
stpy_pcg and stpy_kmv_dxx.  No GPU: the queries touch no device.
"""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_kmv_workspace", os.path.join(HERE, "golden", "make_golden_kmv_workspace.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)


def test_workspace_queries_return_the_recorded_sizes():
	from stpy_amd import _lib
	with open(MG.PATH) as fh:
		golden = json.load(fh)
	got = MG.walks(_lib.load())
	assert sorted({MG.stored_key(name) for name in got}) == sorted(golden) and len(got) == 2 * len(MG.DS) * (4 + len(MG.RS))
	for name, values in got.items():
		want = [v for v, count in golden[MG.stored_key(name)] for _ in range(count)]
		assert len(values) == len(want) == len(MG.TS) * len(MG.SIZES) * (1 if "dtheta" in name or "pcg" in name else len(MG.QS)), name
		first = next((k for k, (a, b) in enumerate(zip(values, want)) if a != b), None)
		assert first is None, (name, "walk index %d" % first, values[first], want[first])
