"""Resumable solves on the GPU (include/snsde.h: snsde_solve_forward_at): a solve cut at step boundaries reproduces the uncut solve
bit for bit on every forward kernel, the offset draws the specified Philox stream, and the front end's extra / extra_solver_state
chain, stream and refuse as documented."""
import warnings

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from oracle import sde_oracle as O
from stable_neural_sdes_amd import _lib, engine
from tests.helpers import assert_kernels, launched_kernels, make_problem, param_spec
from tests.kernel_cases import STEP_OFFSET_CASES, STEP_OFFSET_DT, STEP_OFFSET_L, STEP_OFFSET_TS

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

TS, DT, L, CASES = STEP_OFFSET_TS, STEP_OFFSET_DT, STEP_OFFSET_L, STEP_OFFSET_CASES      # (tests/kernel_cases.py)
CUTS = (0, 3, 9, 16, 22, 37)      # offsets of phase 3, 1, 0, 2 modulo 4; a first piece shorter than a Philox block; cuts inside, on and
                                  # beyond the lean kernel's first 16-step batch
SEED = 0x0123_4567_89AB_CDEF

LEAN_VARIANT = {'lean specialised': 'specialised', 'lean general': 'general', 'lean general milstein': 'general'}


def test_the_cases_cover_every_forward_kernel():
    assert {c.fwd for c in CASES} == set(_lib.FWD_KERNELS) - {'none'}


def _flat(pr):
    spec = param_spec(pr['io'], pr['no'], pr['NL'], pr['C'], pr['H'])
    return torch.from_numpy(np.concatenate([pr['params'][n].reshape(-1) for n, _ in spec])).to(DEV)


class _Problem:
    """The device inputs of a case, built once; call(grid, y0, **kw) describes one solve on them."""

    def __init__(self, c, seed=21):
        self.c = c
        self.pr = pr = make_problem(seed, c.io, c.no, c.NL, c.B, c.H, c.C, c.L)
        self.model = engine.model_struct(c.C, c.H, c.H, c.NL, c.io, c.no)
        self.flat, self.coeffs, self.y0 = _flat(pr), torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['y0']).to(DEV)
        self.grid = engine.step_grid(np.array(c.ts, np.float32), c.dt, pr['times'], torch.device(DEV))

    def call(self, grid, y0, **kw):
        c = self.c
        return engine.SolveCall(self.model, self.flat, self.coeffs, grid, y0.contiguous(), method=c.method, kernel=c.kernel, seed=SEED,
                                row_offset=40, stream_all=c.stream_all, two_tile=c.two_tile, exact_order=c.exact,
                                precision='bf16' if c.bf16 else 'fp32', **kw)


@pytest.mark.parametrize('case', CASES, ids=[c.test for c in CASES])
def test_chunks_reproduce_the_whole(case):
    p = _Problem(case)
    assert p.grid.N == CUTS[-1] and list(p.grid.out_step) == [10, 24, 36]
    plain = p.call(p.grid, p.y0)
    assert_kernels(plain, fwd=case.fwd)
    if case.test in LEAN_VARIANT:
        assert engine.lean_variant(plain) == LEAN_VARIANT[case.test]
    whole = plain.launch().clone()
    assert torch.isfinite(whole).all()
    at0 = p.call(p.grid, p.y0, step_offset=0)      # the keyword at 0 is the call without it
    assert_kernels(at0, fwd=case.fwd)
    assert torch.equal(at0.launch(), whole)
    y, seen = p.y0, []
    for c0, c1 in zip(CUTS[:-1], CUTS[1:]):
        sub, ks = engine.sub_grid(p.grid, c0, c1)
        piece = p.call(sub, y, step_offset=c0)
        assert_kernels(piece, fwd=case.fwd)
        if case.test in LEAN_VARIANT:
            assert engine.lean_variant(piece) == LEAN_VARIANT[case.test]
        ys = piece.launch()
        assert piece.config == p.call(sub, y).config      # the offset is no plan input
        for j, k in enumerate(ks):
            assert torch.equal(ys[1 + j], whole[k]), (case.test, 'output', k, 'of the piece at', c0)
            seen.append(k)
        y = ys[-1].clone()      # the hand-over: the state after step c1 - 1
    assert seen == [1, 2, 3]
    # ... and the pieces do draw other increments than a replay of the beginning would
    sub, _ = engine.sub_grid(p.grid, 22, 37)
    assert not torch.equal(p.call(sub, p.y0, step_offset=22).launch(), p.call(sub, p.y0).launch())


def test_offsets_share_the_configuration_and_its_cached_sizes():
    p = _Problem(CASES[1])
    a = p.call(p.grid, p.y0)
    n = len(engine._SIZE_CACHE)
    b = p.call(p.grid, p.y0, step_offset=12345)
    assert a.config == b.config and len(engine._SIZE_CACHE) == n and b.step_offset == 12345
    assert b.workspace.numel() == a.workspace.numel()
    for bad in (dict(save_act=True, save_traj=True), dict(z0_linear=(torch.zeros(32, 5, device=DEV), torch.zeros(32, device=DEV)))):
        with pytest.raises(ValueError, match='step_offset'):
            p.call(p.grid, p.y0, step_offset=3, **bad)
    big = p.call(p.grid, p.y0, step_offset=2 ** 31 - 1 - 37)      # the largest legal offset solves
    assert torch.isfinite(big.launch()).all()


@pytest.mark.parametrize('case', [CASES[1], CASES[-1]], ids=['mfma', 'generic srk'])
def test_the_offset_draws_the_specified_stream(case):
    p = _Problem(case)
    n0, row_offset, B, H = 6, 1000, case.B, case.H
    call = engine.SolveCall(p.model, p.flat, p.coeffs, p.grid, p.y0, method=case.method, kernel=case.kernel, seed=SEED,
                            row_offset=row_offset, save_dW=True, step_offset=n0)
    assert_kernels(call, fwd=case.fwd)
    call.launch()
    rows = np.arange(row_offset, row_offset + B)
    h = (p.grid.t1 - p.grid.t0).astype(np.float32)
    exp = np.stack([O.philox_normals(SEED, rows, n0 + n, H) * np.sqrt(h[n], dtype=np.float32) for n in range(p.grid.N)])
    got = call.dW_out.cpu().numpy()
    np.testing.assert_allclose(got, exp, rtol=2e-6, atol=2e-7)
    if case.method == 'srk':
        xi = np.stack([O.philox_normals(SEED, rows, n0 + n, H, stream=1) for n in range(p.grid.N)])
        hh = h[:, None, None]
        exp_u = hh * (np.float32(0.5) * exp + np.sqrt(hh / np.float32(12), dtype=np.float32) * xi)
        np.testing.assert_allclose(call.dU_out.cpu().numpy(), exp_u, rtol=2e-6, atol=2e-7)


# ---- the front end ------------------------------------------------------------------------------------------------------------------

TS4 = torch.tensor([0.0, 0.75, 2.25, 4.0])


def _module(io, no, B, H, C_, Lk=7, seed=9, hermite=False):
    pr = make_problem(seed, io, no, 2, B, H, C_, Lk, hermite=hermite)
    m = S.Diffusion_model(C_, H, H, 2, input_option=io, noise_option=no)
    with torch.no_grad():
        for name, q in m.named_parameters():
            q.copy_(torch.from_numpy(pr['params'][name]))
    m = m.to(DEV).requires_grad_(False)
    m.set_X(torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['times']).to(DEV))
    return m, pr


def _chain(m, y0, ts, method, options, first_state=None):
    """The pieces between consecutive entries of ts, each continued from the one before; returns (outputs 0 .., last state)."""
    outs, y, state = [], y0, first_state
    for k in range(len(ts) - 1):
        ys, state = S.sdeint(m, y, ts[k:k + 2], dt=0.25, method=method, options=dict(options), extra=True, extra_solver_state=state)
        outs.append(ys[0] if k == 0 else None)
        outs.append(ys[1])
        y = ys[1]
    return torch.stack([o for o in outs if o is not None]), state


@pytest.mark.parametrize('extra_options', [{}, {'samples': 2}, {'row_offset': 8, 'global_rows': 64}], ids=['plain', 'samples', 'shard'])
@pytest.mark.parametrize('method', ['euler', 'srk'])
@pytest.mark.parametrize('field', ['lean', 'w4'])
def test_sdeint_chained_calls_equal_the_single_call(field, method, extra_options):
    io, no, H, fwd = (4, 17, 32, 'lean' if method == 'euler' else 'general_m4') if field == 'lean' else (3, 18, 64, 'w4')
    m, pr = _module(io, no, 8, H, 5)
    y0 = torch.from_numpy(pr['y0']).to(DEV)
    options = dict(extra_options, seed=77)
    with launched_kernels() as lk:
        whole = S.sdeint(m, y0, TS4.to(DEV), dt=0.25, method=method, options=dict(options))
        got, state = _chain(m, y0, TS4.to(DEV), method, options)
    if 'samples' not in extra_options or field == 'lean':
        assert lk.fwd == [fwd], lk.fwd
    assert state[0].tolist() == [16, 77, 1]
    assert tuple(got.shape) == tuple(whole.shape) and torch.equal(got, whole)
    # the low-level knob is the same continuation
    tail = S.sdeint(m, whole[2], TS4[2:].to(DEV), dt=0.25, method=method, options=dict(options, step_offset=9))
    assert torch.equal(tail[1], whole[3])


def test_a_fresh_call_returns_the_key_it_drew():
    m, pr = _module(4, 17, 8, 32, 5)
    y0, ts = torch.from_numpy(pr['y0']).to(DEV), TS4.to(DEV)
    first, state = S.sdeint(m, y0, ts[:3], dt=0.25, method='euler', extra=True)
    rest = S.sdeint(m, first[-1], ts[2:], dt=0.25, method='euler', extra_solver_state=state)
    steps, key, keyed = state[0].tolist()
    assert (steps, keyed) == (9, 1)
    whole = S.sdeint(m, y0, ts, dt=0.25, method='euler', options={'seed': key})
    assert torch.equal(torch.cat([first, rest[1:]]), whole)


def test_streaming_appends_knots_between_the_pieces():
    m, pr = _module(4, 17, 8, 32, 5, Lk=9, hermite=True)
    y0 = torch.from_numpy(pr['y0']).to(DEV)
    coeffs, times = m.coeffs, m.times
    ts = torch.tensor([0.0, 2.0, 4.0, 6.5, 8.0], device=DEV)
    with launched_kernels() as lk:
        whole = S.sdeint(m, y0, ts, dt=0.25, method='euler', options={'seed': 5})
        m.set_X(coeffs[:, :4].contiguous(), times[:5].contiguous())      # the series as it is known at t = 4
        first, state = S.sdeint(m, y0, ts[:3], dt=0.25, method='euler', options={'seed': 5}, extra=True)
        m.set_X(coeffs, times)                                           # four more observations have arrived
        rest = S.sdeint(m, first[-1], ts[2:], dt=0.25, method='euler', extra_solver_state=state)
    assert lk.fwd == ['lean']
    assert state[0].tolist() == [16, 5, 1]
    assert torch.equal(torch.cat([first, rest[1:]]), whole)


def test_ensemble_members_equal_their_own_continued_solves():
    sdes, prs = zip(*[_module(4, 17, 8, 128, 21, seed=30 + i) for i in range(2)])
    for sde in sdes[1:]:
        sde.set_X(sdes[0].coeffs, sdes[0].times)
    y0 = torch.stack([torch.from_numpy(pr['y0']).to(DEV) for pr in prs])
    ts = TS4.to(DEV)
    with launched_kernels() as lk:
        got = S.sdeint_ensemble(list(sdes), y0, ts, dt=0.25, method='euler', options={'seed': 3, 'step_offset': 6, 'strict': True})
    assert lk.fwd == ['lean'] and tuple(got.shape) == (4, 2, 8, 128)
    for i, sde in enumerate(sdes):
        own = S.sdeint(sde, y0[i], ts, dt=0.25, method='euler',
                       options={'seed': 3, 'step_offset': 6, 'row_offset': 8 * i, 'global_rows': 16})
        assert torch.equal(got[:, i], own)
    assert not torch.equal(got, S.sdeint_ensemble(list(sdes), y0, ts, dt=0.25, method='euler', options={'seed': 3}))


def test_refusals_at_the_front_end():
    m, pr = _module(4, 17, 8, 32, 5)
    y0, ts = torch.from_numpy(pr['y0']).to(DEV), TS4.to(DEV)
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint(m, y0.clone().requires_grad_(True), ts, dt=0.25, method='euler', options={'seed': 1, 'step_offset': 4})
    # Milstein with sqrt(y) noise: no kernel covers it; offset 0 takes the tensor-op loop, a continuation must not
    m7, pr7 = _module(4, 7, 8, 32, 5)
    y7 = torch.from_numpy(pr7['y0']).to(DEV).abs() + 0.1
    with warnings.catch_warnings(), launched_kernels() as lk:
        warnings.simplefilter('ignore')      # (the loop's one warning per configuration)
        looped = S.sdeint(m7, y7, ts, dt=0.25, method='milstein', options={'seed': 1})
    assert tuple(looped.shape) == (4, 8, 32) and lk.fwd == []      # (the launch was refused: no kernel ran, the loop answered)
    with pytest.raises(NotImplementedError, match='fused solve.*caller-supplied `bm`'):
        S.sdeint(m7, y7, ts, dt=0.25, method='milstein', options={'seed': 1, 'step_offset': 4})
