"""tests/buffer_arena.py on CPU tensors: the arena sees one changed guard byte and no write inside a view, the two offsets give the
stated alignment, the allocation proxy fills and counts and restores - and engine.py allocates through nothing the proxy cannot
see, which is the premise of tests/test_gpu_poisoned_allocations.py."""
import inspect
import re
import types

import pytest
import torch

from stable_neural_sdes_amd import engine
from tests.buffer_arena import FILLS, GUARD_BYTES, Arena, fill_bytes, poisoned_allocations, recorded_calls, same_bits


@pytest.mark.parametrize('fill', FILLS)
def test_a_changed_guard_byte_is_seen_and_a_written_view_is_not(fill):
    for side in ('before', 'after'):
        for where in (1, GUARD_BYTES):          # the byte next to the view and the far end of the band
            arena = Arena('cpu', fill, 1 << 16)
            a, b = arena.take(10), arena.take(7, torch.int32, 1)
            a.fill_(1.5)
            b.fill_(-3)
            arena.check('written views')
            first, last = arena.views[1]
            at = first - where if side == 'before' else last + where - 1
            arena.buf[at] ^= 0x10                # one byte, one bit
            with pytest.raises(AssertionError, match='guard bytes changed'):
                arena.check(f'{side} {where}')
    assert float(Arena('cpu', 0x3F, 1 << 14).take(1)[0]) == pytest.approx(0.7470588, abs=1e-6)
    assert torch.isnan(Arena('cpu', 0xFF, 1 << 14).take(1)[0]) and int(Arena('cpu', 0xFF, 1 << 14).take(1, torch.int32)[0]) == -1


def test_views_are_aligned_as_stated_and_do_not_share_a_guard():
    arena = Arena('cpu', 0xFF, 1 << 17)
    last = 0
    for numel, dtype, offset in ((5, torch.float32, 0), (3, torch.float32, 1), (7, torch.uint8, 0), (9, torch.uint8, 1),
                                 (2, torch.int32, 1), (0, torch.float32, 0), (1000, torch.float32, 0)):
        v = arena.take(numel, dtype, offset)
        assert v.numel() == numel and v.dtype == dtype
        assert v.data_ptr() % 256 == 4 * offset and v.data_ptr() % 16 == 4 * offset
        first, end = arena.views[-1]
        assert first - last >= GUARD_BYTES and end + GUARD_BYTES <= arena.buf.numel()
        last = end
    with pytest.raises(AssertionError, match='full'):
        arena.take(1 << 17)


def test_the_proxy_fills_counts_and_restores():
    mod = types.ModuleType('m')
    mod.torch = torch
    for fill in FILLS:
        with poisoned_allocations(mod, fill, keep=True) as proxy:
            assert mod.torch is proxy and mod.torch.float32 is torch.float32 and mod.torch.zeros(2).sum() == 0
            f = mod.torch.empty((3, 5), dtype=torch.float32)
            u = mod.torch.empty(11, dtype=torch.uint8)
            i = mod.torch.empty_like(torch.zeros(4, dtype=torch.int32))
            l = mod.torch.empty((2, 2), dtype=torch.int64)
            z = mod.torch.empty(0)
            assert f.new_empty(0).numel() == 0
            assert proxy.count == 4 and len(proxy.kept) == 4 and z.numel() == 0
            for t in (f, u, i, l):
                assert bool((t.reshape(-1).view(torch.uint8) == fill).all())
        assert mod.torch is torch
    with pytest.raises(RuntimeError):
        with poisoned_allocations(mod, 0xFF):
            raise RuntimeError('inside')
    assert mod.torch is torch
    with poisoned_allocations(engine, 0x3F) as proxy:
        assert engine.torch is proxy
    assert engine.torch is torch and proxy.count == 0
    with recorded_calls(engine) as rec:
        assert engine._ptr(None) is None and engine._ptr(torch.zeros(2)).value
    assert engine.torch is torch and engine._ptr.__module__ == engine.__name__ and not rec.calls
    assert same_bits(fill_bytes(torch.empty(3), 0xFF), fill_bytes(torch.empty(3), 0xFF)) and not same_bits(torch.zeros(1), -torch.zeros(1))


def test_engine_allocates_through_the_patched_name_only():
    """Every uninitialised allocation of engine.py is `torch.empty(` or `torch.empty_like(` through the module's own name `torch`
    - what `poisoned_allocations(engine, ..)` replaces - but the zero-element `new_empty(0)` placeholders; `new_zeros` is
    initialised memory.  A new spelling (Tensor.new_empty(n), empty_strided, a second import of torch, torch.Tensor(..)) fails here."""
    src = inspect.getsource(engine)
    code = '\n'.join(line.split('#')[0] for line in src.splitlines())
    imports = [i.strip() for i in re.findall(r'^\s*(?:import torch\b.*|from torch\b.*)$', code, re.M)]
    # (`import torch.x as y` binds y alone: a submodule, no second name for torch and no allocation function)
    assert all(i == 'import torch' or re.fullmatch(r'import torch\.[\w.]+ as \w+', i) for i in imports) and 'import torch' in imports, imports
    calls = re.findall(r'([\w.]*\bempty\w*)\(([^)]*)', code)
    assert calls, 'engine.py allocates nothing?'
    through = [c for c in calls if c[0] in ('torch.empty', 'torch.empty_like')]
    placeholders = [c for c in calls if c[0].endswith('.new_empty')]
    assert len(through) >= 40 and len(through) + len(placeholders) == len(calls), sorted({c[0] for c in calls})
    assert all(args.strip() == '0' for _, args in placeholders), placeholders
    for banned in (r'\bempty_strided\b', r'\.new\(', r'torch\.\w*Tensor\(', r'\.resize_\(', r'torch\.cuda\.\w*Tensor'):
        assert not re.search(banned, code), banned
    assert len(re.findall(r'\.new_zeros\(', code)) == len(re.findall(r'new_zeros', code))      # (initialised: counted, not banned)
