"""Particle filtering on sample paths on the GPU (include/snsde.h: snsde_sample_resample): the kernel against the float64 numpy
statement of tests/sample_resample_reference.py, the special values, the buffer contract on guarded arenas, determinism and graph
capture, and torchsde.sdeint_filter against the single sampled solve and the by-hand chain.

Bounds (derived in tests/sample_resample_reference.py from the summation order the header documents, unit = 2^-24): ess, logz and
the resampled logw_out within E_ess / E_logz; a kept logw_out equals a bit for bit; the decision wherever ess is not within E_ess
of threshold S; an ancestor equals the reference's wherever the comparison margin min_n |t_j - P_n| / P_{S-1} exceeds delta (about
(S + 15) 2^-24 for even weights, up to 2 S 2^-24 for concentrated ones), and elsewhere differs by at most one and is a live
particle.  The share of (g, j) inside the margin is capped at 2 % per shape and asserted on the reference alone, before the GPU
result is looked at; measured on the CPU with these seeds: at most 1.6 % at S = 255 / 256, 0.8 % at S = 64, 0.003 % at S <= 7.
state_out is compared bit for bit with state gathered by the kernel's own ancestors: no tolerance."""
import functools
import math

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests import sample_resample_reference as R
from tests.buffer_arena import FILLS, Arena, place, recorded_calls, replay, same_bits
from tests.helpers import launched_kernels, make_problem
from tests.kernel_cases import STEP_OFFSET_CASES
from tests.test_sample_resample_cpu import check_special, special_cases, special_state

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(shape, scale):
    return R.make_case(shape, scale)


@functools.lru_cache(maxsize=None)
def _reference(shape, scale, with_inc, stratified, threshold):
    c = _case(shape, scale)
    return R.reference(c['logw'], c['loginc'] if with_inc else None, c['us'] if stratified else c['u'], threshold, stratified)


def _numpy(out):
    return dict(ancestor=out.ancestor.cpu().numpy().astype(np.int64), ess=out.ess.cpu().numpy().astype(np.float64),
                logz=out.logz.cpu().numpy().astype(np.float64), resampled=out.resampled.cpu().numpy().astype(np.int64),
                logw_out=out.log_weight.cpu().numpy())


@pytest.mark.parametrize('scale', R.SCALES)
@pytest.mark.parametrize('shape', R.SHAPES + [R.STRIDE_SHAPE], ids=str)
def test_the_kernel_against_the_reference(shape, scale):
    G, Sn, W = shape
    c = _case(shape, scale)
    modes = [(inc, strat, thr) for inc in (False, True) for strat in (False, True) for thr in R.THRESHOLDS]
    if shape == R.STRIDE_SHAPE:      # (the grid stride is no function of the mode: one of each)
        modes = [(True, False, 0.5), (False, True, 1.0)]
    # the reference alone first: the share of ancestors it cannot pin stays under the cap
    for inc, strat, thr in modes:
        share = R.unpinned_share(_reference(shape, scale, inc, strat, thr))
        assert share <= R.SHARE_CAP, (shape, scale, inc, strat, thr, share)
    state, logw, loginc = _dev(c['state']).reshape(G * Sn, W), _dev(c['logw']), _dev(c['loginc'])
    moved = 0
    for inc, strat, thr in modes:
        ref = _reference(shape, scale, inc, strat, thr)
        out = engine.sample_resample(state, Sn, logw, loginc if inc else None, _dev(c['us'] if strat else c['u']), thr, strat)
        assert out.state.dtype == torch.float32 and out.ancestor.dtype == torch.int32 and out.resampled.dtype == torch.int32
        assert tuple(out.state.shape) == (G * Sn, W) and tuple(out.ancestor.shape) == (G, Sn) and tuple(out.logz.shape) == (G,)
        what = f'{shape} scale={scale} inc={inc} stratified={strat} threshold={thr}'
        moved += R.check_outputs(ref, _numpy(out), thr, Sn, what)
        want = state.reshape(G, Sn, W)[torch.arange(G, device=DEV)[:, None], out.ancestor.long()].reshape(G * Sn, W)
        assert same_bits(out.state, want), what
        if thr <= 0:
            assert int(out.resampled.sum()) == 0 and same_bits(out.state, state), what
        if thr >= 1:
            assert int(out.resampled.sum()) == G, what
    print(f'{shape} scale={scale}: {moved} ancestors inside the margin moved by one')


def test_the_route_and_its_fallbacks():
    c = _case((5, 7, 33), 1.0)
    state, logw, u = _dev(c['state']).reshape(35, 33), _dev(c['logw']), _dev(c['u'])
    fused = engine.sample_resample(state, 7, logw, None, u, 1.0)
    ops = engine.sample_resample_tensor_ops(state, 7, logw, None, u, 1.0)
    assert torch.equal(fused.ancestor, ops.ancestor) and same_bits(fused.state, ops.state)      # (the reference pins every ancestor of this case)
    assert float((fused.logz - ops.logz).abs().max()) <= 1e-5 and float((fused.ess - ops.ess).abs().max()) <= 1e-4
    # float64 and S > 256 take the statement; a non-contiguous state is made contiguous for the kernel
    d = engine.sample_resample(state.double(), 7, logw.double(), None, u.double(), 1.0)
    assert d.state.dtype == torch.float64 and torch.equal(d.ancestor, ops.ancestor)
    wide = engine.sample_resample(torch.zeros(2 * 300, 3, device=DEV), 300, torch.zeros(2, 300, device=DEV), None, torch.full((2,), 0.5, device=DEV), 1.0)
    assert wide.ancestor.tolist() == [list(range(300))] * 2
    strided = state.t().contiguous().t()
    assert not strided.is_contiguous() and same_bits(engine.sample_resample(strided, 7, logw, None, u, 1.0).state, fused.state)
    with pytest.raises(ValueError, match='inference only'):
        engine.sample_resample(state.clone().requires_grad_(True), 7, logw, None, u, 1.0)
    drawn = engine.sample_resample(state, 7, logw, threshold=1.0, generator=torch.Generator(DEV).manual_seed(1))
    again = engine.sample_resample(state, 7, logw, threshold=1.0, generator=torch.Generator(DEV).manual_seed(1))
    assert torch.equal(drawn.ancestor, again.ancestor)
    # the members of an ensemble fold into the groups
    lead = engine.sample_resample(state.reshape(5, 7, 33), 7, logw.reshape(5, 1, 7), None, u.reshape(5, 1), 1.0)
    assert same_bits(lead.state.reshape(35, 33), fused.state) and tuple(lead.ess.shape) == (5, 1)


# ---- special values ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(special_cases()))
def test_special_values_and_isolation(name):
    rows, u, kind = special_cases()[name]
    lw, state, ud = torch.tensor(rows, dtype=torch.float32, device=DEV), special_state().to(DEV), torch.tensor(u, dtype=torch.float32, device=DEV)
    inc = torch.zeros_like(lw)
    for loginc in (None, inc):
        out = engine.sample_resample(state, 4, lw, loginc, ud, 1.0)
        check_special(name, out, lw, state, kind)
        if name == 'dead trailing particles and u just below 1':
            assert out.ancestor[1].tolist()[-1] == 1
        if name == 'dead leading particles and u = 0':
            assert out.ancestor[1].tolist()[0] == 2
        # isolation: the neighbours' bits are the bits of the same groups launched alone
        for g in (0, 2):
            alone = engine.sample_resample(state[4 * g:4 * g + 4].contiguous(), 4, lw[g:g + 1].contiguous(), None if loginc is None else inc[g:g + 1],
                                           ud[g:g + 1].contiguous(), 1.0)
            for field in ('log_weight', 'ancestor', 'ess', 'logz', 'resampled'):
                assert same_bits(getattr(out, field)[g:g + 1], getattr(alone, field)), (name, g, field)
            assert same_bits(out.state[4 * g:4 * g + 4], alone.state), (name, g)
    # stratified, and with the special row not resampled by the threshold either
    strat = engine.sample_resample(state, 4, lw, None, ud[:, None].expand(3, 4).contiguous(), 1.0, True)
    check_special(name, strat, lw, state, kind)
    kept = engine.sample_resample(state, 4, lw, None, ud, 0.0)
    assert kept.resampled.tolist() == [0, 0, 0] and same_bits(kept.state, state) and same_bits(kept.log_weight, lw)


# ---- the buffer contract --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('stratified', [False, True], ids=['systematic', 'stratified'])
@pytest.mark.parametrize('shape', [(5, 7, 33), (3, 6, 8), R.STRIDE_SHAPE], ids=str)
def test_buffer_contract(shape, stratified):
    """Guarded arenas under the three fills, pointers on a 256-byte boundary and 4 bytes past a 16-byte one: the guards stay, the
    inputs are unchanged, every output byte is written (the same bits under every fill) and the unaligned bits are the aligned ones.
    (5, 7, 33): ragged and scalar rows; (3, 6, 8): 16-byte rows that the offset moves to the scalar path; the grid-stride shape."""
    G, Sn, W = shape
    c = _case(shape, 1.0)
    state, logw, loginc = _dev(c['state']).reshape(G * Sn, W), _dev(c['logw']), _dev(c['loginc'])
    u = _dev(c['us'] if stratified else c['u'])
    with recorded_calls(engine) as rec:
        engine.sample_resample(state, Sn, logw, loginc, u, 0.7, stratified)
    torch.cuda.current_stream().synchronize()
    call = rec.named('snsde_sample_resample')
    assert call.rc == 0 and len(call.outputs) == 6
    fn = _lib.lib().snsde_sample_resample
    got = {}
    for offset in (0, 1):
        for fill in FILLS:
            tag = f'{shape} fill {fill:#04x} offset {offset}'
            sizes = [t.numel() * t.element_size() for t in call.tensors.values()]
            arena = Arena(DEV, fill, sum(Arena.room(n) for n in sizes) + (1 << 16))
            placed = place(call, arena, offset)
            assert len(placed) == 10 and all(p.view.data_ptr() % 16 == 4 * offset for p in placed.values())
            rc = replay(fn, call, placed)
            torch.cuda.current_stream().synchronize()
            assert rc == 0, (tag, rc)
            arena.check(tag)
            for p in placed.values():
                if not p.is_output:
                    assert same_bits(p.view, p.original.reshape(-1)), f'{tag}: an input was changed'
            got[offset, fill] = {ptr: p.view.clone() for ptr, p in placed.items() if p.is_output}
            assert len(got[offset, fill]) == 6
    for key, outs in got.items():      # the engine's own result: every fill, both alignments
        for ptr, out in outs.items():
            assert same_bits(out, call.tensors[ptr].reshape(-1)), f'{shape} {key}: an output depends on its memory or on the alignment'


# ---- determinism and graph capture ---------------------------------------------------------------------------------------------------------

def test_two_launches_and_a_captured_graph_give_the_eager_bits():
    shape = (5, 7, 33)
    G, Sn, W = shape
    a, b = _case(shape, 1.0), R.make_case(shape, 4.0, seed=1)
    state = _dev(a['state']).reshape(G * Sn, W)
    logw, u = _dev(a['logw']), _dev(a['u'])
    first = engine.sample_resample(state, Sn, logw, None, u, 1.0)
    second = engine.sample_resample(state, Sn, logw, None, u, 1.0)
    for x, y in zip(first, second):
        assert same_bits(x, y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        engine.sample_resample(state, Sn, logw, None, u, 1.0)      # (warm: nothing is allocated or loaded inside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = engine.sample_resample(state, Sn, logw, None, u, 1.0)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(captured, first):
        assert same_bits(x, y)
    logw.copy_(_dev(b['logw']))      # rewritten in place: the replay reads the new inputs
    u.copy_(_dev(b['u']))
    graph.replay()
    torch.cuda.synchronize()
    eager = engine.sample_resample(state, Sn, logw, None, u, 1.0)
    assert not torch.equal(eager.ancestor, first.ancestor)
    for x, y in zip(captured, eager):
        assert same_bits(x, y)


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------

TS = torch.tensor([0.0, 0.75, 2.25, 4.0])
CASE = STEP_OFFSET_CASES[1]      # 'lean general': the lean 4-row-tile kernel, B = 8, H = 32


def _module():
    c = CASE
    pr = make_problem(9, c.io, c.no, c.NL, c.B, c.H, c.C, 7)
    m = S.Diffusion_model(c.C, c.H, c.H, c.NL, input_option=c.io, noise_option=c.no)
    with torch.no_grad():
        for name, q in m.named_parameters():
            q.copy_(torch.from_numpy(pr['params'][name]))
    m = m.to(DEV).requires_grad_(False)
    m.set_X(torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['times']).to(DEV))
    return m, torch.from_numpy(pr['y0']).to(DEV)


def _likelihood(Sn):
    def fn(k, yk):      # a Gaussian observation of three state components, fused
        obs = torch.full((yk.shape[0] // Sn, 3), 0.1 * k, device=yk.device)
        return engine.sample_loglik(yk[:, :3].contiguous(), Sn, obs, std=0.5, stats=True)[1]
    return fn


def test_the_driver_against_the_single_solve_and_the_chain_by_hand():
    assert CASE.fwd == 'lean' and CASE.B <= 8
    m, y0 = _module()
    Sn, ts = 4, TS.to(DEV)
    options = {'samples': Sn, 'seed': 77}
    with launched_kernels() as lk:
        whole = S.sdeint(m, y0, ts, dt=0.25, method='euler', options=dict(options))
        keep = S.sdeint_filter(m, y0, ts, _likelihood(Sn), method='euler', dt=0.25, options=options, threshold=0.0)
    assert set(lk.fwd) == {'lean'}, lk.fwd
    assert same_bits(keep.ys, whole) and tuple(keep.ys.shape) == (4, CASE.B * Sn, CASE.H)
    run = torch.zeros(CASE.B, Sn, device=DEV)
    for k in (1, 2, 3):
        run = run + _likelihood(Sn)(k, whole[k])
        assert same_bits(keep.log_weight[k], run), k
    assert int(keep.ancestor.ne(torch.arange(Sn, device=DEV, dtype=torch.int32)).sum()) == 0
    # threshold = 1: every piece is the chain sdeint(.., extra_solver_state) -> sample_resample written by hand
    gen = lambda: torch.Generator(DEV).manual_seed(5)
    always = S.sdeint_filter(m, y0, ts, _likelihood(Sn), method='euler', dt=0.25, options=options, threshold=1.0, generator=gen())
    g, y, state, lw = gen(), y0, None, torch.zeros(CASE.B, Sn, device=DEV)
    for k in (1, 2, 3):
        piece, state = S.sdeint(m, y, ts[k - 1:k + 1], dt=0.25, method='euler', options=dict(options), extra=True, extra_solver_state=state)
        assert same_bits(always.ys[k], piece[1]), k
        r = S.sample_resample(piece[1], Sn, lw, _likelihood(Sn)(k, piece[1]), None, 1.0, False, g)
        for name in ('log_weight', 'ancestor', 'ess', 'logz'):
            assert same_bits(getattr(always, name)[k], getattr(r, name)), (k, name)
        assert int(r.resampled.sum()) == CASE.B
        y, lw = r.state, r.log_weight
    assert not torch.equal(always.ys[3], keep.ys[3])
    for out in (keep, always):
        lse = torch.logsumexp(out.log_weight[-1].double(), dim=-1) - math.log(Sn)
        # float32 weights of size |logz|: logsumexp of the stored values against the kernel's own logz, a few roundings of that size
        assert float((lse - out.logz[-1].double()).abs().max()) <= 16 * R.U32 * (1 + float(out.logz[-1].abs().max()) + math.log(Sn))
        assert same_bits(S.filter_paths(out.ys, out.ancestor, Sn)[-1], out.ys[-1])
