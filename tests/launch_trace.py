"""
Launch-trace recorder -- TEST INFRASTRUCTURE ONLY.
Every device launch of the package goes through a typed wrapper of ``stpy_amd._lib`` and ends in ``_lib._launch``.  ``launch_trace()``
replaces the library handle by a stub that only answers size queries, turns ``_launch`` into a no-op and places "the device" on the
CPU, so that any walk over a kernel expression runs to its end without a GPU and without the library, on ordinary CPU tensors; and it
wraps every public wrapper so that each call is appended, in call order, to ``Trace.launches`` as ``[name, args, kwargs]``.
Only attributes of ``stpy_amd._lib`` and of ``torch`` are patched, and all of them are put back when the context ends.

How an argument is recorded
  tensor inside a registered one   {"t": [role, element offset into it, shape, strides]}
  any other tensor                 {"t": ["scratch", shape, dtype]} -- not which one: where scratch comes from is free
  1-D int32, 1-D float <= 64 long  ... with the values appended (column lists, parameter slots, inverse lengthscales)
  scalars, None                    as they are; lists / tuples element by element
``torch.empty`` / ``torch.empty_like`` hand out zeros while the trace runs: no launch writes anything, so without that the values
recorded for a small output vector would be whatever the allocator left there.
"""
import contextlib
import inspect

import torch

from stpy_amd import _lib

NOT_WRAPPED = ("load", "check", "check_async", "device", "stream_ptr", "dtype_code", "ptr", "ld", "to_device", "like_input")
VALUES_UP_TO = 64


class _StubLibrary:
	"""What ``_lib.load()`` returns while tracing: the queries the wrappers size their buffers with, nothing that launches."""

	def __getattr__(self, name):
		if name == "stpy_potrf_winv_elems":
			return lambda n: -(-int(n) // 128) * 128 * 128
		if name.endswith("_bytes"):
			return lambda *args: 64
		if name == "stpy_async_status":
			return lambda *args: 0
		if name == "stpy_lml_batch_max_n":
			return lambda: 512
		if name == "stpy_gemm_nt_splitk_passes":
			return lambda *args: 1
		raise AttributeError("the launch-trace stub has no %s" % name)


class _Stream:
	cuda_stream = 0


def _extent(t):
	"""Elements from the first to one past the last the view can reach."""
	return sum((n - 1) * abs(s) for n, s in zip(t.shape, t.stride())) + 1


class Trace:
	def __init__(self):
		self.launches = []
		self._roles = []

	def register(self, **tensors):
		"""Names the caller's tensors: an argument that lies inside one of them is recorded under that name."""
		for name, t in tensors.items():
			if t is not None:
				self._roles.append((name, t))
		return self

	def _tensor(self, t):
		t = t.detach()
		rec = None
		if t.numel() > 0:
			for name, r in self._roles:
				if r.numel() == 0 or r.dtype != t.dtype or r.untyped_storage().data_ptr() != t.untyped_storage().data_ptr():
					continue
				off = t.storage_offset() - r.storage_offset()
				if off >= 0 and off + _extent(t) <= _extent(r):
					rec = [name, off, list(t.shape), list(t.stride())]
					break
		if rec is None:
			rec = ["scratch", list(t.shape), str(t.dtype).replace("torch.", "")]
		if t.dim() == 1 and (t.dtype == torch.int32 or (t.is_floating_point() and t.numel() <= VALUES_UP_TO)):
			rec.append(t.tolist())
		return {"t": rec}

	def encode(self, v):
		if torch.is_tensor(v):
			return self._tensor(v)
		if isinstance(v, (list, tuple)):
			return [self.encode(e) for e in v]
		if v is None or isinstance(v, (bool, int, float, str)):
			return v
		return repr(v)

	def _wrap(self, name, fn):
		def traced(*args, **kwargs):
			self.launches.append([name, [self.encode(a) for a in args], {k: self.encode(a) for k, a in kwargs.items()}])
			return fn(*args, **kwargs)
		return traced


@contextlib.contextmanager
def launch_trace(**tensors):
	"""``with launch_trace(a=a, out=out) as tr: ...; tr.launches``.  Further tensors can be named later with ``tr.register``."""
	tr = Trace().register(**tensors)
	cpu = torch.device("cpu")
	stub = _StubLibrary()
	patches = [
		(_lib, "load", lambda: stub),
		(_lib, "_launch", lambda name, *args: None),
		(_lib, "device", lambda: cpu),
		(_lib, "stream_ptr", lambda: None),
		(torch.cuda, "current_stream", lambda *args, **kwargs: _Stream()),
		(torch, "empty", torch.zeros),
		(torch, "empty_like", torch.zeros_like),
	]
	for name, fn in sorted(vars(_lib).items()):
		if inspect.isfunction(fn) and fn.__module__ == _lib.__name__ and not name.startswith("_") and name not in NOT_WRAPPED:
			patches.append((_lib, name, tr._wrap(name, fn)))
	saved = [(owner, name, getattr(owner, name)) for owner, name, _ in patches]
	try:
		for owner, name, new in patches:
			setattr(owner, name, new)
		yield tr
	finally:
		for owner, name, old in saved:
			setattr(owner, name, old)


def first_difference(got, want):
	"""None when the two traces are equal, else a message naming the first launch that differs."""
	for i, (g, w) in enumerate(zip(got, want)):
		if g != w:
			return "launch %d differs\n  recorded: %r\n  golden:   %r" % (i, g, w)
	if len(got) != len(want):
		longer, what = (got, "recorded") if len(got) > len(want) else (want, "golden")
		return "%d launches recorded, %d in the golden; first extra one (%s): %r" % (len(got), len(want), what, longer[min(len(got), len(want))])
	return None
