"""Training through continued solves on the GPU (options={'resume_grad': True}, SNSDE_FLAG_RESUME_GRAD; include/snsde.h:
snsde_solve_forward_at, last paragraph).  B = 8 rows, 16 steps of dt = 0.25, cut at step 9 (n0 & 3 == 1: not on a Philox block
boundary) and, for a chain of two cuts, at step 6 as well; Philox increments, one case per adjoint family.

1. The chained differentiable solve returns the states of the uncut one, torch.equal, on the same forward kernel.
2. Regeneration is pinned exactly: the continued piece once with SNSDE_KEEP_INCREMENTS=1 (the adjoint reads the increments the
   forward saved) and once without (the adjoint regenerates them at the offset) - every gradient torch.equal.  The three
   families that regenerate: the general 4-row-tile adjoint, the H = 256 two-tile adjoint, the wave-pair Euler adjoint.
3. Chained against uncut gradients, both held to float64 autograd through the tensor-op loop fed the increments the fused
   forward drew: per tensor, max |chained - ref| <= 2 max |uncut - ref| + FLOOR max |ref| with FLOOR = 1e-5.  Said plainly: for
   most tensors the floor is the larger term (profiles/resume_grad_margins.txt: the uncut error is 1e-7 to 3e-6 of the largest
   entry), so the assertion is in effect "the chained gradient lies within about 1e-5 of the largest entry of float64", ten times
   tighter than the project's 1e-4 (helpers.grad_close, which both are held to as well); twice the uncut error decides only where
   the uncut solve itself is 5e-6 or more off.  The project's gradient tests have no absolute floor of their own to take.  Why
   a floor at all: a gradient is a float32 sum over steps x rows x features (8192 addends of either sign for theta here), its error
   scales with the sum of their magnitudes and not with the result, and for a tensor of ONE element (theta) the uncut error is a
   single draw that can lie anywhere below that scale - theta of the SRK wave-pair case measured 2.4e-6 uncut and 5.8e-6 chained of
   its value, theta of the SRK lean case 3e-8 and 2.5e-7.  1e-5 is ten float32 units (2^-24 = 6e-8) per hundred-odd roundings of
   such a sum's partial results; a piece computed at a wrong offset is off by the size of the gradient itself.  With
   SNSDE_RESUME_GRAD_MARGINS set the measured errors of both are appended to that file.
4. At offset 0 the _at entry points give the bits of the old names; without the flag the C calls refuse an offset."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.helpers import grad_close, launched_kernels, make_problem

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

TIMES = np.array([0.0, 0.6, 1.7, 2.2, 3.9, 4.4, 6.0], np.float32)
DT, B = 0.25, 8
CUT_TS = {(9,): [0.0, 2.25, 4.0], (6, 9): [0.0, 1.5, 2.25, 4.0]}      # the cut times are step boundaries: steps 6 and 9 of 16
TS = CUT_TS[(6, 9)]                                                     # the uncut solve returns the state at every cut
FLOOR = 1e-5
GRAD_TOL = 1e-4
ERR_UNSUPPORTED = -4

# name -> io, no, NL, H, C, method, kernel, forward kernel, adjoint kernel, dL/dcoeffs wanted, the adjoint regenerates, samples
CASES = {
    'lean euler': (4, 17, 2, 32, 5, 'euler', 'mfma4', 'lean', 'general', True, True, 1),
    'general milstein': (4, 17, 2, 32, 5, 'milstein', 'mfma4', 'lean', 'general', True, True, 1),
    'wave pairs euler': (3, 18, 2, 64, 5, 'euler', 'w4', 'w4', 'w4_fused', False, True, 1),      # (no delta planes: no fused dL/dcoeffs)
    'srk lean field': (4, 17, 2, 32, 5, 'srk', 'mfma4', 'general_m4', 'general_srk', True, False, 1),
    'srk wave pairs': (3, 18, 2, 64, 5, 'srk', 'w4', 'w4', 'w4_fused', False, False, 1),
    'two tile h256 milstein': (1, 13, 1, 256, 3, 'milstein', 'mfma4', 'lean_two_tile_h256', 'two_tile_h256', True, True, 1),
    'generic euler': (4, 17, 2, 24, 5, 'euler', 'generic', 'generic', 'generic', True, False, 1),
    'sampled lean euler': (4, 17, 2, 32, 5, 'euler', 'mfma4', 'lean', 'general', True, True, 4),
    # precision='bf16' + bf16_grad: its adjoint is the general kernel, one of the regenerating ones (no bf16 dL/dcoeffs; the float64
    # reference is the project's straight-through statement of the bf16-operand solve)
    'bf16 lean euler': (4, 17, 2, 64, 5, 'euler', 'auto', 'lean_bf16', 'general', False, True, 1),
}
EXTRA_OPTIONS = {'bf16 lean euler': {'precision': 'bf16', 'bf16_grad': True}}
REGENERATING = [n for n, c in CASES.items() if c[10]]


class _ReplayBM:
    def __init__(self, dW, dU=None):
        self.dW, self.dU, self.n = dW, dU, 0

    def __call__(self, ta, tb, return_U=False):
        out, u = self.dW[self.n], None if self.dU is None else self.dU[self.n]
        self.n += 1
        return (out, u) if return_U else out


@functools.lru_cache(maxsize=None)
def _problem(name):
    io, no, NL, H, C_, method, kernel, fwd, rev, coeffs, regen, Sn = CASES[name]
    rows = B // Sn
    pr = make_problem(500 + 7 * io + no + H, io, no, NL, rows, H, C_, len(TIMES), times=TIMES)
    rng = np.random.default_rng(H + no)
    return pr, (0.5 * rng.standard_normal((rows, H))).astype(np.float32), rng.standard_normal((len(TS), B, H)).astype(np.float32)


def _build(name, dtype, device, replicate=False):
    io, no, NL, H, C_, method, kernel, fwd, rev, want_c, regen, Sn = CASES[name]
    pr, y0, _ = _problem(name)
    m = S.Diffusion_model(C_, H, H, NL, input_option=io, noise_option=no)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
    m = m.to(device=device, dtype=dtype)
    coeffs = torch.from_numpy(pr['coeffs']).to(device=device, dtype=dtype).requires_grad_(want_c)
    m.set_X(coeffs.repeat_interleave(Sn, 0) if replicate else coeffs, torch.from_numpy(pr['times']).to(device))
    return m, torch.from_numpy(y0).to(device=device, dtype=dtype).requires_grad_(True), coeffs


def _options(name, **more):
    Sn, kernel = CASES[name][11], CASES[name][6]
    opts = dict(seed=77, kernel=kernel, **more, **EXTRA_OPTIONS.get(name, {}))
    if Sn > 1:
        opts.update(samples=Sn, sample_grad=True)
    return opts


def _grads(m, y0, coeffs):
    out = {'y0': y0.grad, **{n: p.grad for n, p in m.named_parameters()}}
    if coeffs.requires_grad:
        out['coeffs'] = coeffs.grad
    return out


def _solve(name, cuts=(), keep=None):
    """One differentiable solve on the GPU, cut at the global steps `cuts` (none: the uncut solve, without the opt-in), and its
    backward under the case's loss.  Returns (ys at TS, gradients, autograd nodes of the pieces, kernels launched).  keep: a
    list that receives the pieces' saved increments (the caller has set SNSDE_KEEP_INCREMENTS)."""
    method = CASES[name][5]
    m, y0, coeffs = _build(name, torch.float32, DEV)
    w = torch.from_numpy(_problem(name)[2]).to(DEV)
    with launched_kernels() as lk:
        if not cuts:
            ys = S.sdeint(m, y0, torch.tensor(TS, device=DEV), method=method, dt=DT, options=_options(name))
            nodes = [ys.grad_fn]
        else:
            ts = CUT_TS[tuple(cuts)]
            y, state, pieces, nodes = y0, None, [], []
            for a, b in zip(ts[:-1], ts[1:]):
                piece, state = S.sdeint(m, y, torch.tensor([a, b], device=DEV), method=method, dt=DT, options=_options(name, resume_grad=True),
                                        extra=True, extra_solver_state=state)
                nodes.append(piece.grad_fn)
                pieces.append(piece if not pieces else piece[1:])
                y = piece[-1]
            ys = torch.cat(pieces)
            assert state[0].tolist()[0] == 16
        at = [TS.index(t) for t in (TS if not cuts else CUT_TS[tuple(cuts)])]
        (ys * w[at]).sum().backward()
    if keep is not None:
        for node in nodes:
            keep.append((node.call.dW_out, getattr(node.call, 'dU_out', None)))
    return ys.detach(), _grads(m, y0, coeffs), nodes, lk


@functools.lru_cache(maxsize=None)
def _uncut(name):
    return _solve(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """float64 autograd through the tensor-op loop on the CPU, fed the increments the fused uncut forward drew (saved under
    SNSDE_KEEP_INCREMENTS=1; the states of that run are the uncut run's bit for bit)."""
    method, Sn = CASES[name][5], CASES[name][11]
    old = os.environ.get('SNSDE_KEEP_INCREMENTS')
    os.environ['SNSDE_KEEP_INCREMENTS'] = '1'
    try:
        kept = []
        ys, _, _, _ = _solve(name, keep=kept)
    finally:
        if old is None:
            del os.environ['SNSDE_KEEP_INCREMENTS']
        else:
            os.environ['SNSDE_KEEP_INCREMENTS'] = old
    assert torch.equal(ys, _uncut(name)[0])
    dW, dU = kept[0]
    assert dW is not None and tuple(dW.shape) == (16, B, CASES[name][3])
    if name in EXTRA_OPTIONS:      # bf16 operands: the project's straight-through reference (tests/bf16_grad_reference.py), float64
        from tests import bf16_grad_reference as R16
        pr, y0v, w = _problem(name)
        ref, grads = R16.gradients(dict(pr, y0=y0v), TS, DT, dW.cpu().numpy(), w, method)
        return ref, grads
    m, y0, coeffs = _build(name, torch.float64, 'cpu', replicate=True)
    bm = _ReplayBM(dW.double().cpu(), None if dU is None else dU.double().cpu())
    y = y0.repeat_interleave(Sn, 0) if Sn > 1 else y0
    ref = S.sdeint(m, y, torch.tensor(TS, dtype=torch.float64), bm=bm, method=method, dt=DT, options={'backend': 'torch'})
    (ref * torch.from_numpy(_problem(name)[2]).double()).sum().backward()
    return ref.detach(), _grads(m, y0, coeffs)


def _err(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max())


@pytest.mark.parametrize('cuts', [(9,), (6, 9)], ids=['cut 9', 'cuts 6 9'])
@pytest.mark.parametrize('name', list(CASES))
def test_the_chained_solve_against_the_uncut_one(name, cuts):
    fwd, rev = CASES[name][7], CASES[name][8]
    ys_u, g_u, nodes_u, lk_u = _uncut(name)
    ys_c, g_c, nodes_c, lk_c = _solve(name, cuts)
    # the routes: fused nodes on the kernels the case names, the continued pieces with the offset and the flag
    assert lk_u.fwd == [fwd] and lk_u.rev == [rev], (lk_u.fwd, lk_u.rev)
    assert lk_c.fwd == [fwd] and lk_c.rev == [rev], (lk_c.fwd, lk_c.rev)
    assert [n.call.step_offset for n in nodes_c] == [0] + list(cuts)
    assert all(type(n).__name__.startswith('_FusedSolve') for n in nodes_c + nodes_u)
    assert all(bool(n.call.base_flags & _lib.RESUME_GRAD) == (n.call.step_offset != 0) for n in nodes_c)
    if CASES[name][10]:      # (the adjoint of these pieces regenerated its increments: none were saved)
        assert all(n.call.dW_out is None for n in nodes_c)
    # 1. the states
    at = [TS.index(t) for t in CUT_TS[tuple(cuts)]]
    assert torch.equal(ys_c, ys_u[at]), name
    # 3. the gradients, both against float64 (the uncut solve's loss weighs the state at every cut time: the loss of the two-cut chain)
    if cuts != (6, 9):
        return
    ys_r, g_r = _reference(name)
    # (bf16 operands: an operand that rounds to the other bf16 neighbour moves a row's trajectory and its gradients - what
    #  tests/test_gpu_bf16_grad.py sets rows aside for; the chained and the uncut run share their forward bit for bit, so the bound of 3
    #  holds between them whatever that deviation is, and the 1e-4 against the reference is that file's business, not asked here)
    bf16 = name in EXTRA_OPTIONS
    assert bf16 or _err(ys_u, ys_r) <= 1e-4 * float(ys_r.abs().max())
    assert set(g_c) == set(g_u) == set(g_r)
    for key, ref in g_r.items():
        if ref is None:      # a parameter this field does not read: no gradient from autograd, an exact zero from the fused pass
            assert all(g[key] is None or not bool(g[key].any()) for g in (g_c, g_u)), (name, key)
            continue
        scale = float(ref.abs().max())
        eu, ec = _err(g_u[key], ref), _err(g_c[key], ref)
        if os.environ.get('SNSDE_RESUME_GRAD_MARGINS'):
            with open(os.environ['SNSDE_RESUME_GRAD_MARGINS'], 'a') as fh:
                fh.write(f'{name!r} {key} max|ref| {scale:.3e} uncut {eu:.3e} chained {ec:.3e} bound {2 * eu + FLOOR * scale:.3e}\n')
        print(f'{name} {key}: uncut {eu:.3e} chained {ec:.3e} of max |ref| {scale:.3e}')
        if not bf16:
            grad_close(g_u[key], ref, key, GRAD_TOL, name + ' uncut')
            grad_close(g_c[key], ref, key, GRAD_TOL, name + ' chained')
        assert ec <= 2 * eu + FLOOR * scale, (name, key, 'chained', ec, 'uncut', eu, 'max |ref|', scale)


@pytest.mark.parametrize('name', REGENERATING)
def test_regeneration_at_an_offset_is_pinned_exactly(name, monkeypatch):
    """The continued piece from step 9 on, alone: with the saved increments and with regenerated ones - the same bits everywhere."""
    method = CASES[name][5]
    start = _uncut(name)[0][TS.index(2.25)]
    w = torch.from_numpy(_problem(name)[2]).to(DEV)[2:]
    runs = []
    for keep in (True, False):
        if keep:
            monkeypatch.setenv('SNSDE_KEEP_INCREMENTS', '1')
        else:
            monkeypatch.delenv('SNSDE_KEEP_INCREMENTS', raising=False)
        m, _, coeffs = _build(name, torch.float32, DEV)
        y = start.clone().requires_grad_(True)
        opts = _options(name, resume_grad=True, step_offset=9)
        with launched_kernels() as lk:
            ys = S.sdeint(m, y, torch.tensor([2.25, 4.0], device=DEV), method=method, dt=DT, options=opts)
            (ys * w).sum().backward()
        assert lk.rev == [CASES[name][8]]
        assert (ys.grad_fn.call.dW_out is not None) == keep and ys.grad_fn.call.step_offset == 9
        runs.append((ys.detach(), _grads(m, y, coeffs)))
    (ys_a, g_a), (ys_b, g_b) = runs
    assert torch.equal(ys_a, ys_b) and torch.equal(ys_a[-1], _uncut(name)[0][-1])
    for key in g_a:
        assert (g_a[key] is None) == (g_b[key] is None)
        if g_a[key] is not None:
            assert torch.equal(g_a[key], g_b[key]), (name, key, float((g_a[key] - g_b[key]).abs().max()))
    assert float(g_a['y0'].abs().max()) > 0


def _training_call(step_offset=0, resume_grad=False):
    io, no, NL, H, C_ = CASES['lean euler'][:5]
    pr = make_problem(3, io, no, NL, B, H, C_, len(TIMES), times=TIMES)
    m = S.Diffusion_model(C_, H, H, NL, input_option=io, noise_option=no)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
    m = m.to(DEV)
    m.set_X(torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['times']).to(DEV))
    model, layout, numel = engine.recognise(m)
    grid = engine.step_grid(np.array([0.0, 4.0], np.float32), DT, TIMES, torch.device(DEV))
    return engine.SolveCall(model, engine.flatten_params(m, layout, numel, torch.device(DEV)), torch.from_numpy(pr['coeffs']).to(DEV), grid,
                            torch.from_numpy(pr['y0']).to(DEV), seed=5, kernel='mfma4', save_traj=True, save_act=True,
                            step_offset=step_offset, resume_grad=resume_grad)


def test_at_offset_zero_the_at_entry_points_give_the_bits_of_the_old_names():
    call = _training_call()
    ys = call.launch()
    g = torch.randn_like(ys)
    L, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    adj, grad = engine.backward_with_gradients(call, g, adj0_only=False)
    b, pws = call.bwd_desc, call.keep_pg[0]
    adj2, grad2 = torch.full_like(adj, float('nan')), torch.full_like(grad, float('nan'))
    b.adj = C.c_void_p(adj2.data_ptr())
    assert L.snsde_backward_with_gradients_at(C.byref(b), C.c_void_p(grad2.data_ptr()), C.c_void_p(pws.data_ptr()), pws.numel(), 0, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(adj, adj2) and torch.equal(grad, grad2)
    adj3 = torch.full_like(adj, float('nan'))
    b.adj = C.c_void_p(adj3.data_ptr())
    assert L.snsde_solve_backward_at(C.byref(b), 0, stream) == 0
    adj4 = torch.full_like(adj, float('nan'))
    b.adj = C.c_void_p(adj4.data_ptr())
    assert L.snsde_solve_backward(C.byref(b), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(adj3, adj) and torch.equal(adj4, adj)
    # without the flag an offset is refused by the backward calls and, with training planes, by the forward - before any launch
    assert not call.base_flags & _lib.RESUME_GRAD
    assert L.snsde_solve_backward_at(C.byref(b), 5, stream) == ERR_UNSUPPORTED
    assert L.snsde_backward_with_gradients_at(C.byref(b), C.c_void_p(grad2.data_ptr()), C.c_void_p(pws.data_ptr()), pws.numel(), 5, stream) == ERR_UNSUPPORTED
    assert L.snsde_solve_forward_at(C.byref(call.desc), 5, stream) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(adj4, adj) and torch.equal(grad, grad2)


def test_the_engine_call_takes_the_offset_with_training_planes_under_the_opt_in_only():
    with pytest.raises(ValueError, match='step_offset != 0 is inference only'):
        _training_call(step_offset=3)
    call = _training_call(step_offset=3, resume_grad=True)
    assert call.step_offset == 3 and call.base_flags & _lib.RESUME_GRAD and call.act_save is not None
    assert not _training_call(resume_grad=False).base_flags & _lib.RESUME_GRAD


def _chained_and_uncut(build, method, seed):
    """(uncut, chained with cuts at steps 6 and 9) of a module whose solve is one _ComposedSolve node per call (the zero-padded
    model, a tutorial-style field): each (states, gradients, the node's calls).  build(dtype, device) -> (module, y0 leaf)."""
    w = torch.randn(len(TS), B, build(torch.float32, 'cpu')[1].shape[1], generator=torch.Generator().manual_seed(2)).to(DEV)

    def node_call(ys):      # (the padded route slices the node's output: walk to the node)
        fn = ys.grad_fn
        while not hasattr(fn, 'call'):
            fn = fn.next_functions[0][0]
        return fn.call

    def run(cut):
        m, y0 = build(torch.float32, DEV)
        if not cut:
            ys = S.sdeint(m, y0, torch.tensor(TS, device=DEV), method=method, dt=DT, options={'seed': seed})
            calls = [node_call(ys)]
        else:
            y, state, pieces, calls = y0, None, [], []
            for a, b in zip(TS[:-1], TS[1:]):
                piece, state = S.sdeint(m, y, torch.tensor([a, b], device=DEV), method=method, dt=DT, options={'seed': seed, 'resume_grad': True},
                                        extra=True, extra_solver_state=state)
                calls.append(node_call(piece))
                pieces.append(piece if not pieces else piece[1:])
                y = piece[-1]
            ys = torch.cat(pieces)
        (ys * w).sum().backward()
        return ys.detach(), {'y0': y0.grad, **{n: p.grad for n, p in m.named_parameters()}}, calls

    return run(False), run(True), w


def _against_float64(build, method, uncut, chained, w, tag, exact_states=True):
    """The increments the pieces kept are the uncut solve's, torch.equal (these nodes always keep them: the offset pinned exactly), the
    states too (exact_states) - and both runs against float64 autograd through the tensor-op loop on those increments: the bound of 3."""
    (ys_u, g_u, calls_u), (ys_c, g_c, calls_c) = uncut, chained
    assert [c.step_offset for c in calls_c] == [0, 6, 9] and calls_u[0].step_offset == 0
    assert torch.equal(torch.cat([c.dW_out for c in calls_c]), calls_u[0].dW_out), (tag, 'the pieces drew other increments')
    if exact_states:
        assert torch.equal(ys_c, ys_u), tag
    H = ys_u.shape[-1]
    dW = calls_u[0].dW_out[..., :H].double().cpu()
    assert tuple(dW.shape) == (16, B, H)
    m, y0 = build(torch.float64, 'cpu')
    ref = S.sdeint(m, y0, torch.tensor(TS, dtype=torch.float64), bm=_ReplayBM(dW), method=method, dt=DT, options={'backend': 'torch'})
    (ref * w.double().cpu()).sum().backward()
    g_r = {'y0': y0.grad, **{n: p.grad for n, p in m.named_parameters()}}
    for key, r in g_r.items():
        if r is None:
            assert all(g[key] is None or not bool(g[key].any()) for g in (g_c, g_u)), (tag, key)
            continue
        scale, eu, ec = float(r.abs().max()), _err(g_u[key], r), _err(g_c[key], r)
        print(f'{tag} {key}: uncut {eu:.3e} chained {ec:.3e} of max |ref| {scale:.3e}')
        grad_close(g_u[key], r, key, GRAD_TOL, tag + ' uncut')
        grad_close(g_c[key], r, key, GRAD_TOL, tag + ' chained')
        assert ec <= 2 * eu + FLOOR * scale, (tag, key, 'chained', ec, 'uncut', eu, 'max |ref|', scale)


def test_the_zero_padded_route_takes_the_offset():
    """H = 24 under kernel='auto' is solved zero-padded to H = 32 by its own autograd node (it keeps its increments): the chained solve
    returns the uncut states, and both runs' gradients are held to float64 as in 3."""
    assert engine.padding_plan(engine.model_struct(5, 24, 24, 2, 4, 17), B, len(TIMES), 16, 'euler') is not None
    pr = make_problem(21, 4, 17, 2, B, 24, 5, len(TIMES), times=TIMES)

    def build(dtype, device):
        m = S.Diffusion_model(5, 24, 24, 2, input_option=4, noise_option=17)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
        m = m.to(device=device, dtype=dtype)
        m.set_X(torch.from_numpy(pr['coeffs']).to(device=device, dtype=dtype), torch.from_numpy(pr['times']).to(device))
        return m, torch.from_numpy(pr['y0']).to(device=device, dtype=dtype).requires_grad_(True)

    uncut, chained, w = _chained_and_uncut(build, 'euler', 9)
    assert uncut[2][0].model.hidden_channels == 32      # (the padded model)
    _against_float64(build, 'euler', uncut, chained, w, 'zero padded')


@pytest.mark.parametrize('kind,method', [('lnsde', 'euler'), ('gsde', 'milstein')])
def test_a_tutorial_style_field_takes_the_offset(kind, method):
    """A composed (tutorial-style) field trains through _sdeint_composed's own node: a continued differentiable piece draws the
    increments of the global steps - the pieces' saved increments are the uncut solve's, torch.equal - and the gradients hold to
    float64 as in 3.  The states are NOT bit-equal on this route, cut or not, training or inference: the time-only diffusion factor
    is tabulated per call by the module's own g_net in tensor ops, and a library GEMM over 16 rows and over 6, 3 and 7 rows rounds a
    row differently (measured: one float32 unit in the table, 3.6e-7 in states of size 1.8; the inference chain of the parent differs
    likewise).  A table entry one unit off moves a step's diffusion term by 2^-24 of it; over sixteen steps, with the drift's growth a
    small factor, the states stay within 1e-5 of the largest one (160 units) - a piece on the wrong noise is off by the state's size."""
    from stable_neural_sdes_amd import fields
    from tests.tutorial_fields import TutorialField
    pr = make_problem(31, 4, 17, 2, B, 32, 3, len(TIMES), times=TIMES)
    torch.manual_seed(4)
    proto = TutorialField(kind, 3, 32, 1, 'lipswish')
    with torch.no_grad():
        for p in proto.parameters():
            p.mul_(1.5)
    y0v = torch.rand(B, 32, generator=torch.Generator().manual_seed(6)) * 0.5 + 0.25

    def build(dtype, device):
        m = TutorialField(kind, 3, 32, 1, 'lipswish')
        m.load_state_dict(proto.state_dict())
        m = m.to(device=device, dtype=dtype)
        m.set_X(torch.from_numpy(pr['coeffs']).to(device=device, dtype=dtype), torch.from_numpy(pr['times']).to(device=device, dtype=dtype))
        return m, y0v.clone().to(device=device, dtype=dtype).requires_grad_(True)

    assert fields.compose(build(torch.float32, DEV)[0]) is not None
    loop = S.torchsde._sdeint_torch
    S.torchsde._sdeint_torch = lambda *a, **k: (_ for _ in ()).throw(AssertionError('fell back to the generic stepper'))
    try:
        uncut, chained, w = _chained_and_uncut(build, method, 13)
    finally:
        S.torchsde._sdeint_torch = loop
    assert all(bool(c.base_flags & _lib.RESUME_GRAD) == (c.step_offset != 0) for c in chained[2])
    _against_float64(build, method, uncut, chained, w, f'tutorial {kind}', exact_states=False)
    diff, scale = float((chained[0] - uncut[0]).abs().max()), float(uncut[0].abs().max())
    print(f'tutorial {kind}: chained states within {diff:.3e} of the uncut ones (largest {scale:.3e})')
    assert diff <= 1e-5 * scale, (kind, diff, scale)
