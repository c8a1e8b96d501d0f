"""
The launch plan of the kernel expression, pinned without a GPU: for every (expression, entry point) pair of the catalogue in
tests/golden/make_golden_launch_trace.py the sequence of ``_lib`` wrapper calls -- which entry point, on which operands, with which
scalars, in which order -- equals the one recorded in tests/golden/T1_launch_trace.json.  A change to how the expression is walked
that changes a launch shows up here, before it goes near a device; an intended change regenerates the file (see the generator).
"""
import importlib.util
import json
import os

import pytest
import torch

from stpy_amd import _lib
from tests.launch_trace import first_difference, launch_trace

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_launch_trace", os.path.join(HERE, "golden", "make_golden_launch_trace.py"))
catalogue = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(catalogue)

ENTRIES = catalogue.entries()


@pytest.fixture(scope="module")
def golden_trace():
	with open(catalogue.PATH) as fh:
		return json.load(fh)


def test_catalogue_and_golden_hold_the_same_entries(golden_trace):
	assert [name for name, _ in ENTRIES] == list(golden_trace)


@pytest.mark.parametrize("name,fn", ENTRIES, ids=[name for name, _ in ENTRIES])
def test_launch_trace_matches_golden(name, fn, golden_trace):
	got = catalogue.record(fn)
	assert len(got) > 0 or name.endswith("/self_grad_into")          # (only the self term of a stationary kernel launches nothing)
	diff = first_difference(got, golden_trace[name])
	if diff is not None:
		print("%s: %s" % (name, diff))
	assert diff is None, "%s: %s" % (name, diff)


def test_patches_are_undone():
	before = {k: v for k, v in vars(_lib).items()}
	empty, empty_like, stream = torch.empty, torch.empty_like, torch.cuda.current_stream
	with pytest.raises(RuntimeError, match="inside"):
		with launch_trace():
			assert _lib.device() == torch.device("cpu")
			raise RuntimeError("inside")
	assert {k: v for k, v in vars(_lib).items()} == before
	assert (torch.empty, torch.empty_like, torch.cuda.current_stream) == (empty, empty_like, stream)


def _hessian_call(k):
	t = catalogue.data()
	G = torch.full((catalogue.Q, catalogue.D), 3.0, dtype=torch.float64)
	H = torch.full((catalogue.Q, catalogue.D, catalogue.D), 3.0, dtype=torch.float64)
	with launch_trace(x=t["a"], xt=t["b"], G=G, H=H) as tr:
		try:
			k._grad_into(t["a"], t["b"], G, alpha=t["alpha"], H=H)
		finally:
			# refused before anything is touched: nothing launched, G and H as they were
			assert tr.launches == [] and bool((G == 3.0).all()) and bool((H == 3.0).all())


def test_hessian_of_a_product_kernel_is_refused():
	with pytest.raises(NotImplementedError, match=r"Hessian of a product kernel \(item joined by '\*'\) is not implemented on the device"):
		_hessian_call(catalogue.se() * catalogue.matern())


@pytest.mark.parametrize("make,what", [
	(lambda: catalogue.matern(0.5), r"Hessian of the Matern nu=0\.5 term is not defined \(singular at r = 0\)"),
	(lambda: catalogue.matern(1.5), r"Hessian of the Matern nu=1\.5 term is not defined \(singular at r = 0\)"),
	(lambda: catalogue.se() + catalogue.KF(kernel_name="full_covariance_matern", nu=1.5, d=catalogue.D),
	 r"Hessian of the Matern nu=1\.5 \(full covariance\) term is not defined \(singular at r = 0\)"),
], ids=["matern12", "matern32", "se+fc_matern32"])
def test_hessian_of_a_rough_matern_term_is_refused(make, what):
	with pytest.raises(NotImplementedError, match=what):
		_hessian_call(make())
