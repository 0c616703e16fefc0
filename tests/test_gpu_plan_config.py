"""engine.SolveConfig on the GPU: a SolveCall asks the library with the configuration engine.query_descriptor asks with, and the
memo of the host-side size queries, keyed by the record, serves each A/B switch its own sizes.

Shapes: H = 64, C = 3, 8 knots, 6 steps, 24 rows - M = 3 members of 8 rows, S = 2 paths per input row, 24 / S / M = 4 coefficient
rows: the smallest at which `members` with `samples` passes SolveCall's own checks.  The switch pairs run 8 rows at H = 256
(stream_all) and H = 128 (two_tile)."""
import ctypes as C
import signal

import numpy as np
import pytest
import torch

from stable_neural_sdes_amd import _lib, engine

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

KNOTS, STEPS, CH, B, M, S = 8, 6, 3, 24, 3, 2
FIELDS = ('batch', 'knots', 'n_steps', 'method', 'kernel', 'flags', 'members', 'samples', 'global_rows', 'row_offset')
# (SolveCall keywords; the engine.query_descriptor keywords that say the same are derived in _query_options)
OPTION_SETS = {
    'plain': {},
    'bf16': dict(precision='bf16'),
    'sampled': dict(samples=S),
    'sampled training': dict(samples=S, sample_grad=True, save_traj=True, save_act=True),
    'ensemble': dict(members=M),
    'ensemble training': dict(members=M, ensemble_grad=True, save_traj=True, save_act=True),
    'ensemble samples': dict(members=M, samples=S, ensemble_samples=True),
    'ensemble nets': dict(members=M, ensemble_nets=True),
    'ensemble nets grad': dict(members=M, ensemble_grad=True, ensemble_nets=True, ensemble_nets_grad=True),
    'opt-ins without carriers': dict(sample_grad=True, bf16_grad=True, ensemble_grad=True, ensemble_samples=True, ensemble_nets=True,
                                     ensemble_nets_grad=True),
    'supplied dW': dict(dW=True),
    'row_out': dict(row_out=True),
    'global_rows': dict(global_rows=48, row_offset=8),
    'srk exact order': dict(method='srk', exact_order=True, lean_general=True),
}


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('plan-config GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _grid():
    times = np.linspace(0.0, float(STEPS), KNOTS).astype(np.float32)
    return engine.step_grid(np.array([0.0, 2.5, float(STEPS)], np.float32), 1.0, times, torch.device(DEV))


def _call(H, rows, seed=3, **options):
    """A SolveCall of `rows` rows at hidden size H on random parameters, coefficients and initial states; dW=True / row_out=True
    stand for a supplied tensor of the right shape."""
    model = engine.model_struct(CH, H, H, 2, 4, 17)
    gen = torch.Generator().manual_seed(seed)
    members, samples = options.get('members', 0) or 1, options.get('samples', 0) or 1
    numel = _lib.param_layout(model)[1]
    flat = (0.1 * torch.randn((members, numel) if members > 1 else (numel,), generator=gen)).to(DEV)
    coeffs = (0.1 * torch.randn((rows // samples // members, KNOTS - 1, 4 * CH), generator=gen)).to(DEV)
    y0 = (0.1 * torch.randn((rows, H), generator=gen)).to(DEV)
    grid = _grid()
    if options.get('dW'):
        options['dW'] = (0.1 * torch.randn((grid.N, rows, H), generator=gen)).to(DEV)
    if options.get('row_out'):
        options['row_out'] = (torch.arange(rows, dtype=torch.int32) % grid.T).to(DEV)
    return model, engine.SolveCall(model, flat, coeffs, grid, y0, seed=11, **options)


def _query_options(options):
    q = {k: v for k, v in options.items() if k not in ('dW', 'row_out', 'save_traj', 'save_act')}
    q['training'] = bool(options.get('save_traj') or options.get('save_act'))
    return q


@pytest.mark.parametrize('name', list(OPTION_SETS))
def test_a_solvecall_asks_with_the_configuration_of_the_query(name):
    options = dict(OPTION_SETS[name])
    model, call = _call(64, B, **dict(options))
    query = engine.query_descriptor(model, B, KNOTS, STEPS, **_query_options(options))
    assert call.grid.N == STEPS
    for f in FIELDS:
        assert getattr(call.desc, f) == getattr(query, f), (name, f, getattr(call.desc, f), getattr(query, f))
    assert call.base_flags == query.flags == call.config.flags
    for f in ('noise_table', 'traj', 'act_save'):      # (the optional pointers a query can ask with)
        assert bool(getattr(call.desc, f)) == bool(getattr(query, f)), (name, f)
    for f in ('dW', 'row_out'):                        # (... and the two it cannot: present exactly where supplied)
        assert bool(getattr(call.desc, f)) == bool(options.get(f)) == getattr(call.config, f), (name, f)
    assert not call.desc.seed_dev and not call.config.seed_dev
    assert call.cfg_key is call.config and call.members == (options.get('members', 0) or 1)
    assert isinstance(call.delta_slots, int) and (call.act_save is not None or call.delta_slots == 0)


def _direct_sizes(call):
    """Workspace bytes and save layout of the call's own descriptor, asked of the library directly."""
    slots, planes, dslots = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().snsde_save_layout(C.byref(call.desc), C.byref(slots), C.byref(planes), C.byref(dslots)), 'snsde_save_layout')
    return max(int(_lib.lib().snsde_workspace_bytes(C.byref(call.desc))), 256), slots.value, dslots.value


@pytest.mark.parametrize('H, switch, kernels', [(256, 'stream_all', ('lean_two_tile_h256', 'lean_streamed_h256')),
                                                (128, 'two_tile', ('lean', 'lean_two_tile_h128'))])
def test_each_switch_gets_its_own_sizes_and_the_same_bits(H, switch, kernels):
    engine._SIZE_CACHE.clear()
    calls = [_call(H, 8, save_traj=True, save_dW=True, save_act=True, **{switch: on})[1] for on in (False, True)]
    assert calls[0].config != calls[1].config and calls[0].config == calls[1].config.replace(**{switch: False})
    assert tuple(engine.forward_kernel(c) for c in calls) == kernels
    for c in calls:
        ws, slots, dslots = _direct_sizes(c)
        assert (c.workspace.numel(), c.act_save.shape[1], c.delta_slots) == (ws, slots, dslots)
        assert engine._SIZE_CACHE[('fwd', c.config)] == int(_lib.lib().snsde_workspace_bytes(C.byref(c.desc)))
    ys = [c.launch().clone() for c in calls]
    torch.cuda.synchronize()
    assert torch.isfinite(ys[0]).all() and torch.equal(ys[0], ys[1])
