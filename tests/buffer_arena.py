"""Memory the tests control, for the buffer contracts of include/snsde.h ("every element of grad_ys is written", "no workspace",
"the caller zero-fills what no job writes").  Plain helpers, importable without a GPU.

The package allocates every output, saved plane and workspace with torch.empty, and the caching allocator hands a second call the
block the first one freed - still holding the first call's correct values.  So "two launches, the same bits" inside one process
cannot see an element a kernel forgot to write or a workspace word it read before writing, and nobody's assertion owns the tensor
next to an output.  Three tools close that:

`Arena`                  views with a guard band of GUARD_FLOATS floats on both sides, cut from ONE allocation that is filled bytewise
                         with `fill`: an overrun shorter than the band lands in memory the test owns and check() reports it.
`FILLS`                  0x00 the control; 0xFF a NaN as float, -1 as int32, the largest size_t; 0x3F 0.747.. as float - finite and
                         plausible, because a stale NaN can be masked (fmaxf(NaN, 0) = 0 equals the zero arm).
`poisoned_allocations`   the name `torch` inside a module replaced by a proxy whose empty / empty_like return the real allocation
                         filled bytewise; everything else forwards.
`recorded_calls`         the C calls a function of the engine makes, with the tensor behind every pointer and which of them the
                         function allocated (its outputs and workspaces), so `replay` can make the same call - the same scalars,
                         flags and NULL pointers - with every device pointer moved into an Arena."""
import contextlib
import ctypes as C

import torch

GUARD_FLOATS = 1024                 # 4 KiB on both sides of every view: a condition, not a measurement
GUARD_BYTES = 4 * GUARD_FLOATS
FILLS = (0x00, 0xFF, 0x3F)
ALIGN = 256                         # offset_floats = 0: the view starts on a 256-byte boundary


def fill_bytes(t, fill):
    """Every byte of the storage behind a freshly allocated tensor = fill (one fill kernel: capturable)."""
    torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).fill_(fill)
    return t


def bits(t):
    """The bytes of a tensor as a flat uint8 tensor: comparisons on it count NaN payloads and signed zeros."""
    return t.contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class Arena:
    """Arena(device, fill).take(numel, dtype, offset_floats) -> a view of `numel` elements inside one allocation filled with `fill`,
    GUARD_BYTES of fill on both sides.  offset_floats = 0: on a 256-byte boundary; 1: 4 bytes past a 16-byte boundary (past the
    256-byte one).  check() asserts that every byte outside the views - the guards and the unused rest - still equals fill."""

    def __init__(self, device, fill, capacity=1 << 22):
        self.fill = int(fill)
        self.buf = torch.full((capacity,), self.fill, dtype=torch.uint8, device=device)
        self._cursor = 0
        self.views = []             # (first byte, one past the last byte)

    @staticmethod
    def room(nbytes):
        """Bytes of arena one view of nbytes takes at most."""
        return nbytes + 2 * GUARD_BYTES + ALIGN + 16

    def take(self, numel, dtype=torch.float32, offset_floats=0):
        nbytes = int(numel) * torch.empty(0, dtype=dtype).element_size()
        start = self._cursor + GUARD_BYTES
        start += -(self.buf.data_ptr() + start) % ALIGN
        start += 4 * offset_floats
        end = start + nbytes
        assert end + GUARD_BYTES <= self.buf.numel(), f'arena of {self.buf.numel()} bytes is full'
        self._cursor = end + GUARD_BYTES
        self.views.append((start, end))
        return self.buf[start:end].view(dtype)

    def check(self, what=''):
        bad = self.buf != self.fill
        for a, b in self.views:
            bad[a:b] = False
        n = int(bad.count_nonzero())
        if n:
            at = int(bad.nonzero()[0])
            near = min(range(len(self.views)), key=lambda i: min(abs(at - self.views[i][0]), abs(at - self.views[i][1])))
            a, b = self.views[near]
            side = f'{a - at} bytes before its first' if at < a else f'{at - b} bytes past its last'
            raise AssertionError(f'{what}: {n} guard bytes changed (fill {self.fill:#04x}); the first at byte {at}, {side} byte of '
                                 f'view {near} ({b - a} bytes)')


class _TorchProxy:
    """Stands in for the name `torch` inside a module: empty / empty_like fill what they allocate, the rest is torch."""

    def __init__(self, real, fill, keep):
        self._real, self.fill = real, fill
        self.count = 0                              # allocations filled (zero-element tensors are left alone)
        self.kept = [] if keep else None            # ... and the tensors themselves, in order

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _poison(self, t):
        if t.numel():
            if self.fill is not None:
                fill_bytes(t, self.fill)
            self.count += 1
            if self.kept is not None:
                self.kept.append(t)
        return t

    def empty(self, *a, **k):
        return self._poison(self._real.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._poison(self._real.empty_like(*a, **k))


@contextlib.contextmanager
def poisoned_allocations(module, fill, keep=False):
    """Inside the block `module.torch` is a proxy whose empty / empty_like return the real allocation filled bytewise with `fill`
    (None: counted, not filled).  Yields the proxy: .count allocations filled, .kept the tensors (keep=True)."""
    real = module.torch
    proxy = _TorchProxy(real, fill, keep)
    module.torch = proxy
    try:
        yield proxy
    finally:
        module.torch = real


# ---- the C calls of an engine function, recorded and replayed on guarded memory ---------------------------------------------------

class RecordedCall:
    def __init__(self, name, args, rc, tensors, outputs):
        self.name, self.args, self.rc = name, args, rc
        self.tensors = tensors          # data_ptr -> the tensor the engine passed there
        self.outputs = outputs          # data_ptrs the engine allocated for this call: outputs and workspaces


class _LibProxy:
    """Stands in for the name `_lib` inside a module: lib() returns the library with every snsde_* call recorded."""

    def __init__(self, real, rec):
        self._real, self._rec = real, rec

    def __getattr__(self, name):
        return getattr(self._real, name)

    def lib(self):
        return _Library(self._real.lib(), self._rec)


class _Library:
    def __init__(self, lib, rec):
        self._lib, self._rec = lib, rec

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('snsde_'):
            return fn

        def call(*args):
            rc = fn(*args)
            self._rec._add(name, args, rc)
            return rc
        return call


class Recording:
    def __init__(self):
        self.calls, self._tensors, self._proxy, self._mark = [], {}, None, 0

    def _ptr(self, t):
        if t is None:
            return None
        self._tensors[t.data_ptr()] = t
        return C.c_void_p(t.data_ptr())

    def _add(self, name, args, rc):
        if name.endswith('_bytes'):     # a size query between two allocations of the call that follows: it owns none of them
            return
        new = self._proxy.kept[self._mark:]
        self._mark = len(self._proxy.kept)
        self.calls.append(RecordedCall(name, args, rc, dict(self._tensors), {t.data_ptr() for t in new}))

    def named(self, name):
        got = [c for c in self.calls if c.name == name]
        assert len(got) == 1, (name, [c.name for c in self.calls])
        return got[0]


@contextlib.contextmanager
def recorded_calls(module):
    """Inside the block every `_lib.lib().snsde_*` call of `module` is recorded with its arguments, the tensor behind every pointer
    that went through `module._ptr`, and the tensors `module` allocated (torch.empty / empty_like) since the call before."""
    rec = Recording()
    real_lib, real_ptr = module._lib, getattr(module, '_ptr', None)
    with poisoned_allocations(module, None, keep=True) as proxy:
        rec._proxy = proxy
        module._lib = _LibProxy(real_lib, rec)
        if real_ptr is not None:
            module._ptr = rec._ptr
        try:
            yield rec
        finally:
            module._lib = real_lib
            if real_ptr is not None:
                module._ptr = real_ptr


def _pointer_value(a):
    if a is None:
        return None
    if isinstance(a, C.c_void_p):
        return a.value
    return int(a)


class Placed:
    """One tensor of a recorded call moved into an arena: `view` is what the replayed call reads or writes."""

    def __init__(self, original, view, is_output):
        self.original, self.view, self.is_output = original, view, is_output
        self.workspace = is_output and original.dtype == torch.uint8


def place(call, arena, offset_floats, extra=None, pointer_args=()):
    """Every tensor of a recorded call in `arena`: inputs copied, outputs and workspaces left holding the fill.
    -> {data_ptr: Placed}.  extra: {data_ptr: (tensor, is_output)} for pointers that did not go through module._ptr;
    pointer_args: as for `replay`."""
    known = {p: (t, p in call.outputs) for p, t in call.tensors.items()}
    known.update(extra or {})
    placed = {}

    def visit(value):
        if value is None or value in placed:
            return
        assert value in known, f'{call.name}: a device pointer the recording does not know ({value:#x})'
        t, is_output = known[value]
        view = arena.take(t.numel(), t.dtype, offset_floats)
        if not is_output:
            view.copy_(t.reshape(-1))
        placed[value] = Placed(t, view, is_output)

    for value in _device_pointers(call, pointer_args):
        visit(value)
    return placed


def _struct_of(a):
    obj = getattr(a, '_obj', a)         # C.byref(x) keeps x as ._obj
    if isinstance(obj, C.Structure):
        return [obj]
    if isinstance(obj, C.Array) and issubclass(obj._type_, C.Structure):
        return list(obj)
    return None


def _pointer_fields(s):
    return [n for n, tp in s._fields_ if tp is C.c_void_p]


def _device_pointers(call, pointer_args=()):
    """The device pointers of a recorded call, in argument order: every c_void_p argument but the last (the stream), and the
    c_void_p fields of a struct (or array of structs) argument."""
    for i, a in enumerate(call.args[:-1]):
        structs = _struct_of(a)
        if structs is not None:
            for s in structs:
                for n in _pointer_fields(s):
                    yield getattr(s, n)
        elif a is None or isinstance(a, C.c_void_p) or i in pointer_args:
            yield _pointer_value(a)


def replay(fn, call, placed, pointer_args=()):
    """The recorded call again through `fn` (the ctypes function), every device pointer replaced by its arena view.
    pointer_args: positions whose plain-int argument is a device pointer (a caller that passed data_ptr() itself)."""
    keep, args = [], []
    move = lambda v: None if v is None else placed[v].view.data_ptr()
    for i, a in enumerate(call.args):
        structs = _struct_of(a)
        if i == len(call.args) - 1:
            args.append(a)
        elif structs is not None:
            obj = getattr(a, '_obj', a)
            copy = type(obj).from_buffer_copy(obj)
            for s in ([copy] if isinstance(copy, C.Structure) else copy):
                for n in _pointer_fields(s):
                    setattr(s, n, move(getattr(s, n)))
            keep.append(copy)
            args.append(C.byref(copy) if hasattr(a, '_obj') else copy)
        elif a is None or isinstance(a, C.c_void_p):
            args.append(None if a is None else C.c_void_p(move(a.value)))
        elif i in pointer_args:
            args.append(move(int(a)))
        else:
            args.append(a)
    return fn(*args)
