"""snsde_solve::global_rows on the host: every planning query answers for a batch shard what it answers for the whole problem.
Host-only queries of the library (the style of tests/test_routes_cpu.py), the Python option's resolution, no GPU compute."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.global_rows_cases import (FOUR_ROW, KNOTS, SHARDS, STEPS, elementwise_model, flip_batch, net_model, path)
from tests.golden.make_route_golden import ANSWERS, FIELDS, TRAIN, _row, solve_struct
from tests.helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _answers(row, global_rows=0, row_offset=0):
    """make_route_golden.answers for a descriptor with global_rows / row_offset set."""
    lib = _lib.lib()
    s = solve_struct(row)
    s.global_rows, s.row_offset = global_rows, row_offset
    b = _lib.Backward()
    b.fwd = s
    a, p, d = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = lib.snsde_save_layout(C.byref(s), C.byref(a), C.byref(p), C.byref(d))
    return [lib.snsde_forward_path(C.byref(s)), lib.snsde_backward_supported(C.byref(s)), lib.snsde_workspace_bytes(C.byref(s)),
            lib.snsde_backward_workspace_bytes(C.byref(b)), rc, a.value, p.value, d.value,
            lib.snsde_param_gradients_workspace_bytes(C.byref(b))]


@pytest.mark.parametrize('H', [32, 64, 128, 256])
def test_a_shard_planned_with_global_rows_takes_the_whole_problems_tiles(H):
    """At the first batch N where `auto` leaves the 4-row tiles, an N / 8-row shard takes them again - unless it is planned with
    global_rows = N.  (The second assertion is the one that fails without the feature.)"""
    model, N = elementwise_model(H), flip_batch(H)
    whole = path(model, N)
    assert whole == 'mfma16'
    assert path(model, N // SHARDS) in FOUR_ROW and path(model, N // SHARDS) != whole
    for r in (0, 3, SHARDS - 1):
        assert path(model, N // SHARDS, global_rows=N, row_offset=r * (N // SHARDS)) == whole
    # the lean-instantiation query plans from the same number: a 16-row plan launches no lean kernel
    s = _lib.Solve()
    s.model, s.batch, s.knots, s.n_steps, s.n_out, s.global_rows = model, N // SHARDS, KNOTS, STEPS, 2, N
    assert _lib.LEAN_VARIANTS[_lib.lib().snsde_lean_variant(C.byref(s))] == 'none'
    s.global_rows = 0
    if H != 256:
        assert _lib.LEAN_VARIANTS[_lib.lib().snsde_lean_variant(C.byref(s))] != 'none'
    # a whole problem small enough for 4-row tiles keeps its shards there
    assert path(model, N // SHARDS, global_rows=N - 32) in FOUR_ROW


def test_wave_pair_shards_follow_the_whole_problems_plan():
    """H = 64 with a diffusion net under Euler: 8192 rows run 16-row tiles, a 1024-row shard alone the wave pairs."""
    model = net_model()
    assert path(model, 1024) == 'w4'
    assert path(model, 8192) == 'mfma16'
    assert path(model, 1024, global_rows=8192, row_offset=7168) == path(model, 8192)
    assert path(model, 1024, global_rows=6144) == 'w4'
    # ... and the other way round: a 16-row-sized shard of nothing larger than itself is unchanged
    assert path(model, 8192, global_rows=8192) == 'mfma16'


@pytest.mark.parametrize('method', [0, 2])
def test_backward_queries_agree_with_the_forward_plan(method):
    """snsde_backward_supported, snsde_save_layout and the workspace queries with global_rows set: the global plan's kernel at the
    LOCAL batch - exactly what the same shard answers with that kernel pinned by hand."""
    srk = ('srk_tab',) if method == 2 else ()
    # wave pairs -> 16-row tiles (Euler); under SRK the net has no 16-row flavour: the wave pairs at every size, but the fused
    # wave-pair adjoint only up to 6144 rows of the problem
    shard = _row(3, 64, 2, 1, 18, 1024, method, knots=KNOTS, n_steps=STEPS, ptrs=TRAIN + srk)
    whole = _row(3, 64, 2, 1, 18, 8192, method, knots=KNOTS, n_steps=STEPS, ptrs=TRAIN + srk)
    alone, planned, big = (dict(zip(ANSWERS, a)) for a in (_answers(shard), _answers(shard, 8192, 2048), _answers(whole)))
    assert alone['delta_slots'] == 0 and alone['backward_supported'] == 1             # the fused wave-pair adjoint
    assert planned['backward_supported'] == big['backward_supported'] == 1
    for k in ('forward_path', 'save_layout_rc', 'act_slots', 'stage_planes', 'delta_slots'):
        assert planned[k] == big[k], k
    assert planned['delta_slots'] > 0
    if method == 0:
        pinned = dict(zip(ANSWERS, _answers(_row(3, 64, 2, 1, 18, 1024, 0, kernel=3, knots=KNOTS, n_steps=STEPS, ptrs=TRAIN))))
        assert planned == pinned
    else:
        assert planned['forward_path'] == alone['forward_path'] == _lib.PATHS.index('w4')
    assert planned['backward_workspace_bytes'] < big['backward_workspace_bytes']      # sized for the local rows


@pytest.mark.parametrize('H', [32, 64, 128, 256])
def test_elementwise_shard_answers_are_the_pinned_kernels(H):
    N = flip_batch(H)
    shard = _row(3, H, 2, 4, 17, N // SHARDS, 0, knots=KNOTS, n_steps=STEPS, ptrs=TRAIN)
    pinned = _row(3, H, 2, 4, 17, N // SHARDS, 0, kernel=3, knots=KNOTS, n_steps=STEPS, ptrs=TRAIN)
    assert _answers(shard, N, N - N // SHARDS) == _answers(pinned)
    assert _answers(shard) != _answers(pinned)


def test_zero_and_own_batch_change_no_answer_of_the_route_fixture():
    """global_rows = 0 and global_rows = batch: every query of every descriptor of tests/golden/routes.npz answers as without."""
    g = load('routes.npz')
    assert tuple(g['fields']) == FIELDS
    seen = set()
    for row in g['desc']:
        d = dict(zip(FIELDS, (int(v) for v in row)))
        base = _answers(row)
        assert _answers(row, d['batch']) == base, d
        seen.add((d['H'], d['method']))
    assert len(seen) >= 15


def test_global_rows_smaller_than_the_shards_last_row_is_refused():
    model = elementwise_model(64)
    assert path(model, 256, global_rows=255) == 'none'
    assert path(model, 256, global_rows=300, row_offset=64) == 'none'
    assert path(model, 256, global_rows=320, row_offset=64) != 'none'
    row = _row(3, 64, 2, 4, 17, 256, 0, knots=KNOTS, n_steps=STEPS, ptrs=TRAIN)
    bad = dict(zip(ANSWERS, _answers(row, 300, 64)))
    assert bad['save_layout_rc'] == -2 and bad['backward_supported'] == 0 and bad['forward_path'] == 0      # SNSDE_ERR_DIMS
    assert dict(zip(ANSWERS, _answers(row, -5)))['save_layout_rc'] == -2
    # the launch entry point validates before it touches a buffer
    s = solve_struct(row)
    s.n_out, s.global_rows, s.row_offset = 2, 300, 64
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys'):
        setattr(s, f, C.c_void_p(4096))
    assert _lib.lib().snsde_solve_forward(C.byref(s), None) == -2


def test_sdeint_refuses_a_global_rows_below_the_shard():
    pr_B, H = 6, 16
    m = S.Diffusion_model(3, H, H, 2, input_option=4, noise_option=17)
    times = torch.arange(5, dtype=torch.float32)
    m.set_X(torch.zeros(pr_B, 4, 12), times)
    y0 = torch.zeros(pr_B, H)
    with pytest.raises(ValueError, match='global_rows'):
        S.sdeint(m, y0, times, dt=1.0, method='euler', options={'global_rows': 5})
    with pytest.raises(ValueError, match='global_rows'):
        S.sdeint(m, y0, times, dt=1.0, method='euler', options={'global_rows': 8, 'row_offset': 4})
    with pytest.raises(ValueError, match='global_rows'):
        S.sdeint(m, y0, times, dt=1.0, method='euler', options={'global_rows': 'galaxy'})
    with pytest.raises(ValueError, match='global_rows'):
        engine.resolve_global_rows(7, 4, 4)
    # the tensor loop has no tiles: the option is accepted and ignored there
    a = S.sdeint(m, y0, times, dt=1.0, method='euler', options={'backend': 'torch', 'seed': 3, 'global_rows': 48, 'row_offset': 6})
    b = S.sdeint(m, y0, times, dt=1.0, method='euler', options={'backend': 'torch', 'seed': 3})
    assert torch.equal(a, b)


def test_resolution_without_a_process_group_and_the_sharding_helper():
    assert engine.resolve_global_rows(None, 12) == 0 and engine.resolve_global_rows(0, 12) == 0
    assert engine.resolve_global_rows('world', 12) == 12
    assert engine.resolve_global_rows(96, 12, 84) == 96
    assert S.sharding.shard_plan_options(11, 2, 1) == {'row_offset': 6, 'global_rows': 11}
    assert S.sharding.shard_plan_options(4096, 8, 3) == {'row_offset': 1536, 'global_rows': 4096}


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _world_worker(rank, world, port, out_q):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from stable_neural_sdes_amd import engine as E
        from tests.global_rows_cases import elementwise_model as em, flip_batch as fb, path as pth
        N = fb(128)
        local = N // world
        g = E.resolve_global_rows('world', local, rank * local)
        out_q.put((rank, g, pth(em(128), local, global_rows=g, row_offset=rank * local), pth(em(128), local)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_world_resolves_to_world_size_times_the_local_batch_under_gloo():
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_world_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    N = flip_batch(128)
    assert [g[1] for g in got] == [N, N]
    assert all(g[2] == 'mfma16' and g[3] in FOUR_ROW for g in got)
