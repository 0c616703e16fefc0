"""The adjoint of the resampling step on the GPU (include/snsde.h: snsde_sample_resample_backward).

grad_state is compared bit for bit with a sequential sum over the children in ascending j done on the host in float32: the kernel
only moves and adds, in the order the header states.  grad_a is compared with the float64 restatement
    c = resampled ? grad_logz + sum_j grad_logw_out[j] : grad_logz,   grad_a[n] = c e_n / P_{S-1}   (kept: + grad_logw_out[n])
within a bound built from the pieces tests/sample_resample_reference.py derives for the forward's logz and ess (unit = 2^-24,
x_n = mx - a_n): e_n is within e_n (x_n + 6) unit and P_{S-1} within BP of their exact values - the same e_n and the same chain -
the quotient and the product round once each, and c is a sequential float32 sum of S + 1 terms, within unit S (|grad_logz| +
sum |grad_logw_out|).  So
    |grad_a[n] - exact| <= 1.01 (w_n (|c| ((x_n + 6) unit + BP / P + 2 unit) + E_c) + unit |exact|)
the last term for the one rounded addition of a kept row.  The measured error is printed in units of this bound."""
import functools
import math

import numpy as np
import pytest
import torch

from stable_neural_sdes_amd import _lib, engine
from tests import sample_resample_reference as R
from tests.buffer_arena import FILLS, Arena, place, recorded_calls, replay, same_bits
from tests.test_sample_resample_grad_cpu import check_special_gradients, special_gradients
from tests.test_sample_resample_cpu import special_cases

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

# (G, S, W): one particle; a scalar row; a 16-byte row; the largest S; several packs of 64 groups with a ragged last pack
SHAPES = [(3, 1, 4), (5, 8, 6), (4, 32, 8), (2, 256, 4), (70, 4, 3)]
MODES = [(strat, thr) for strat in (False, True) for thr in (0.0, 0.5, 1.0)]
MIXED = 0.19      # of the five groups of (5, 8, 6), whose ess are 2.46, 1.68, 1.66, 1.05 and 1.38, this threshold resamples the last two


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded inputs of a shape and the three output gradients (float32 numpy)."""
    c = R.make_case(shape, 4.0)
    G, Sn, W = shape
    rng = np.random.default_rng(17 + G + Sn + W)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    c.update(gso=f(G, Sn, W), glw=f(G, Sn), glz=f(G))
    return c


def host_grad_state(gso, anc, res):
    """Row n = the rows of its children added in ascending j, in float32, the first one moved; a kept group is the identity; an
    ancestor outside [0, S) is nobody's child.  gso (G, S, W) float32 or None, anc (G, S), res (G)."""
    G, Sn = anc.shape
    out = np.zeros((G, Sn, 1 if gso is None else gso.shape[2]), np.float32)
    if gso is None:
        return out
    for g in range(G):
        if not res[g]:
            out[g] = gso[g]
            continue
        seen = set()
        for j in range(Sn):
            n = int(anc[g, j])
            if 0 <= n < Sn:
                out[g, n] = (out[g, n] + gso[g, j]).astype(np.float32) if n in seen else gso[g, j]
                seen.add(n)
    return out


def exact_grad_a(c, with_inc, res, glw, glz):
    """(the float64 restatement of grad_a, its bound) for summed groups; res: the decision the backward was handed."""
    ref = R.reference(c['logw'], c['loginc'] if with_inc else None, c['u'], 0.0, False)
    e, a64 = ref['e'], ref['a'].astype(np.float64)
    G, Sn = e.shape
    tot, P = e.sum(1), np.cumsum(e, axis=1)
    w = e / tot[:, None]
    g64 = np.zeros((G, Sn)) if glw is None else glw.astype(np.float64)
    z64 = np.zeros(G) if glz is None else glz.astype(np.float64)
    cc = np.where(res.astype(bool), z64 + g64.sum(1), z64)
    exact = np.where(res.astype(bool)[:, None], cc[:, None] * w, g64 + cc[:, None] * w)
    with np.errstate(all='ignore'):
        x = np.where(e > 0, a64.max(1, keepdims=True) - a64, 0.0)
    BP = R.U32 * (P.sum(1) + (e * (x + 6.0)).sum(1))
    Ec = R.U32 * Sn * (np.abs(z64) + np.abs(g64).sum(1))
    bound = 1.01 * (w * (np.abs(cc)[:, None] * ((x + 6.0) * R.U32 + (BP / tot)[:, None] + 2 * R.U32) + Ec[:, None]) + R.U32 * np.abs(exact)) + 1e-300
    return exact, bound


def _backward(c, shape, with_inc, anc, res, gso=True, glw=True, glz=True):
    G, Sn, W = shape
    return engine.sample_resample_backward(_dev(c['gso']).reshape(G * Sn, W) if gso else None, _dev(c['glw']) if glw else None,
                                           _dev(c['glz']) if glz else None, _dev(c['logw']), _dev(c['loginc']) if with_inc else None,
                                           anc, res, (Sn, W))


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_the_kernel_against_the_host_sum_and_the_restatement(shape):
    G, Sn, W = shape
    c = _case(shape)
    state, logw, loginc = _dev(c['state']).reshape(G * Sn, W), _dev(c['logw']), _dev(c['loginc'])
    worst = 0.0
    for strat, thr in MODES:
        for with_inc in (True, False):
            what = f'{shape} stratified={strat} threshold={thr} inc={with_inc}'
            fwd = engine.sample_resample(state, Sn, logw, loginc if with_inc else None, _dev(c['us'] if strat else c['u']), thr, strat)
            anc, res = fwd.ancestor.cpu().numpy(), fwd.resampled.cpu().numpy()
            assert thr != 1.0 or res.all()
            assert thr != 0.0 or not res.any()
            gs, ga = _backward(c, shape, with_inc, fwd.ancestor, fwd.resampled)
            assert tuple(gs.shape) == (G * Sn, W) and tuple(ga.shape) == (G, Sn) and gs.dtype == ga.dtype == torch.float32
            want = host_grad_state(c['gso'], anc, res)
            assert same_bits(gs.cpu(), torch.from_numpy(want).reshape(G * Sn, W)), what
            exact, bound = exact_grad_a(c, with_inc, res, c['glw'], c['glz'])
            err = np.abs(ga.cpu().numpy().astype(np.float64) - exact) / bound
            worst = max(worst, float(err.max()))
            assert err.max() <= 1.0, (what, 'grad_a in units of its bound', float(err.max()))
    print(f'{shape}: grad_a at most {worst:.3f} of its bound')


def test_null_gradients_are_zeros():
    shape = (5, 8, 6)
    G, Sn, W = shape
    c = _case(shape)
    fwd = engine.sample_resample(_dev(c['state']).reshape(G * Sn, W), Sn, _dev(c['logw']), _dev(c['loginc']), _dev(c['u']), MIXED)
    assert 0 < int(fwd.resampled.sum()) < G      # (both kinds of group)
    res = fwd.resampled.cpu().numpy()
    full = _backward(c, shape, True, fwd.ancestor, fwd.resampled)
    gs, ga = _backward(c, shape, True, fwd.ancestor, fwd.resampled, gso=False)
    assert same_bits(gs, torch.zeros_like(gs)) and same_bits(ga, full[1])
    gs, ga = _backward(c, shape, True, fwd.ancestor, fwd.resampled, glw=False, glz=False)
    assert same_bits(gs, full[0]) and same_bits(ga, torch.zeros_like(ga))
    for glw, glz in ((True, False), (False, True)):
        gs, ga = _backward(c, shape, True, fwd.ancestor, fwd.resampled, glw=glw, glz=glz)
        exact, bound = exact_grad_a(c, True, res, c['glw'] if glw else None, c['glz'] if glz else None)
        assert (np.abs(ga.cpu().numpy() - exact) <= bound).all()


@pytest.mark.parametrize('shape', [(5, 8, 6), (4, 32, 8), (70, 4, 3)], ids=str)
def test_ancestors_that_are_neither_monotone_nor_in_range(shape):
    """ancestor is a caller's input: any int32.  An entry outside [0, S) is the child of nobody - compared, never an index."""
    G, Sn, W = shape
    c = _case(shape)
    rng = np.random.default_rng(3)
    anc = rng.integers(0, Sn, (G, Sn)).astype(np.int32)      # with repeats, in no order
    out_of_range = np.array([-1, Sn, Sn + 5, 2 ** 31 - 1, -2 ** 31, 256, -Sn], np.int32)
    mask = rng.random((G, Sn)) < 0.3
    anc[mask] = rng.choice(out_of_range, int(mask.sum()))
    anc[0] = Sn + 1                                            # a group no row of which has a child
    res = np.ones(G, np.int32)
    res[-1] = 0                                                # a kept group ignores its ancestors
    gs, ga = _backward(c, shape, True, _dev(anc), _dev(res))
    want = host_grad_state(c['gso'], anc, res)
    assert same_bits(gs.cpu(), torch.from_numpy(want).reshape(G * Sn, W))
    assert same_bits(gs[:Sn], torch.zeros(Sn, W, device=DEV))
    exact, bound = exact_grad_a(c, True, res, c['glw'], c['glz'])
    assert (np.abs(ga.cpu().numpy() - exact) <= bound).all()


# ---- special rows ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(special_cases()))
def test_special_rows(name):
    got = special_gradients(engine.sample_resample, name, torch.float32, DEV)
    check_special_gradients(name, *got)
    # a NaN in the output gradient of the state reaches the row of its ancestor and nothing else
    out, gx, gl, cs, cw, cz = special_gradients(engine.sample_resample, name, torch.float32, DEV, nan_row=2)
    parent = int(out.ancestor[0, 2])
    assert torch.isnan(gx).reshape(-1, 3).any(dim=1).nonzero().flatten().tolist() == [parent], name
    assert same_bits(gl, got[2]), name
    # isolation: the neighbours' gradients are those of a run whose row 1 is ordinary
    plain = special_gradients(engine.sample_resample, 'a -Inf weight is never an ancestor', torch.float32, DEV)
    for g in (0, 2):
        assert same_bits(got[1][g], plain[1][g]) and same_bits(got[2][g], plain[2][g]), (name, g)


def test_the_autograd_route_is_the_kernel():
    shape = (5, 8, 6)
    G, Sn, W = shape
    c = _case(shape)
    leaves = [_dev(c['state']).reshape(G * Sn, W).requires_grad_(True), _dev(c['logw']).requires_grad_(True), _dev(c['loginc']).requires_grad_(True)]
    plain = engine.sample_resample(leaves[0].detach(), Sn, leaves[1].detach(), leaves[2].detach(), _dev(c['u']), MIXED)
    with recorded_calls(engine) as rec:
        out = engine.sample_resample(*leaves[:1], Sn, *leaves[1:], _dev(c['u']), MIXED, differentiable=True)
        for a, b in zip(out, plain):      # the forward values of the plain call, bit for bit
            assert same_bits(a.detach(), b)
        assert not (out.ancestor.requires_grad or out.ess.requires_grad or out.resampled.requires_grad)
        got = torch.autograd.grad([out.state, out.log_weight, out.logz], leaves, [_dev(c['gso']).reshape(G * Sn, W), _dev(c['glw']), _dev(c['glz'])])
    assert [call.name for call in rec.calls] == ['snsde_sample_resample', 'snsde_sample_resample_backward']
    gs, ga = _backward(c, shape, True, out.ancestor, out.resampled)
    assert same_bits(got[0], gs) and same_bits(got[1], ga) and same_bits(got[2], ga)
    # only logz is used: the other two gradients are NULL to the kernel
    out = engine.sample_resample(*leaves[:1], Sn, *leaves[1:], _dev(c['u']), MIXED, differentiable=True)
    gx, gl, gi = torch.autograd.grad(out.logz.sum(), leaves)
    soft = torch.softmax((leaves[1] + leaves[2]).detach().double(), dim=-1)
    assert same_bits(gx, torch.zeros_like(gx)) and float((gl.double() - soft).abs().max()) <= 1e-5
    # the statement in tensor ops on the same device gives the same gradients up to round-off
    assert R.unpinned_share(R.reference(c['logw'], c['loginc'], c['u'], MIXED, False)) == 0.0      # (every ancestor of this case is pinned)
    ops = engine.sample_resample_tensor_ops(*leaves[:1], Sn, *leaves[1:], _dev(c['u']), MIXED, differentiable=True)
    assert torch.equal(ops.ancestor, out.ancestor)
    want = torch.autograd.grad([ops.state, ops.log_weight, ops.logz], leaves, [_dev(c['gso']).reshape(G * Sn, W), _dev(c['glw']), _dev(c['glz'])])
    assert float((want[0] - got[0]).abs().max()) <= 1e-5 and float((want[1] - got[1]).abs().max()) <= 1e-5


# ---- determinism and the buffer contract ----------------------------------------------------------------------------------------------------

def test_two_launches_give_the_same_bits():
    for shape in ((4, 32, 8), (70, 4, 3)):
        G, Sn, W = shape
        c = _case(shape)
        fwd = engine.sample_resample(_dev(c['state']).reshape(G * Sn, W), Sn, _dev(c['logw']), _dev(c['loginc']), _dev(c['us']), 1.0, True)
        first = _backward(c, shape, True, fwd.ancestor, fwd.resampled)
        second = _backward(c, shape, True, fwd.ancestor, fwd.resampled)
        assert same_bits(first[0], second[0]) and same_bits(first[1], second[1])


@pytest.mark.parametrize('shape', [(5, 8, 6), (4, 32, 8), (70, 4, 3)], ids=str)
def test_buffer_contract(shape):
    """Guarded arenas under the three fills, pointers on a 256-byte boundary and 4 bytes past a 16-byte one: the guards stay, the
    inputs are unchanged, every output byte is written (the same bits under every fill) and the unaligned bits are the aligned ones
    ((4, 32, 8): 16-byte rows that the offset moves to the scalar path)."""
    G, Sn, W = shape
    c = _case(shape)
    fwd = engine.sample_resample(_dev(c['state']).reshape(G * Sn, W), Sn, _dev(c['logw']), _dev(c['loginc']), _dev(c['u']), 0.7)
    with recorded_calls(engine) as rec:
        _backward(c, shape, True, fwd.ancestor, fwd.resampled)
    torch.cuda.current_stream().synchronize()
    call = rec.named('snsde_sample_resample_backward')
    assert call.rc == 0 and len(call.outputs) == 2
    fn = _lib.lib().snsde_sample_resample_backward
    got = {}
    for offset in (0, 1):
        for fill in FILLS:
            tag = f'{shape} fill {fill:#04x} offset {offset}'
            sizes = [t.numel() * t.element_size() for t in call.tensors.values()]
            arena = Arena(DEV, fill, sum(Arena.room(n) for n in sizes) + (1 << 16))
            placed = place(call, arena, offset)
            assert len(placed) == 9 and all(p.view.data_ptr() % 16 == 4 * offset for p in placed.values())
            rc = replay(fn, call, placed)
            torch.cuda.current_stream().synchronize()
            assert rc == 0, (tag, rc)
            arena.check(tag)
            for p in placed.values():
                if not p.is_output:
                    assert same_bits(p.view, p.original.reshape(-1)), f'{tag}: an input was changed'
            got[offset, fill] = {ptr: p.view.clone() for ptr, p in placed.items() if p.is_output}
            assert len(got[offset, fill]) == 2
    for key, outs in got.items():      # the engine's own result: every fill, both alignments
        for ptr, out in outs.items():
            assert same_bits(out, call.tensors[ptr].reshape(-1)), f'{shape} {key}: an output depends on its memory or on the alignment'
