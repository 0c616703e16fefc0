"""Training through model ensembles on the GPU: options={'ensemble_grad': True} (SNSDE_FLAG_ENSEMBLE_GRAD) against the ordinary
differentiable sdeint of each member run as a shard of the whole (members = 0, its own parameters, row_offset + m Bm, the same
global_rows) - states, dL/dy0 and every parameter gradient member by member, torch.equal, no tolerance: each member is planned as
its own solve (adjoint workgroups, partial-sum blocks, weight-gradient tiles and splits), so every sum runs in the member's own
order.  Every case first asserts, on the descriptor it launches, that ONE forward launch with members = M ran with the flag bit set
and which forward and adjoint kernel it names, and that the member-alone references ran the same kernels with members = 0: the loop
of M solves cannot stand in silently.

Shapes: those of tests/test_gpu_ensemble.py - M = 3 members with different parameters, Bm = 8 rows per member (two 4-row tiles, so
tile -> member is not the identity; one case at Bm = 4), nine irregular knots, eight steps of dt = 1, output times inside the
steps, Philox under a fixed seed, C = 3."""
import signal

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.helpers import assert_kernels, assert_parity, grad_close, make_problem

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

TIMES = np.array([0.0, 0.6, 1.7, 2.2, 3.9, 4.4, 6.0, 6.9, 8.0], np.float32)      # L = 9 knots
TS = np.array([0.0, 2.5, 5.3, 8.0], np.float32)                                  # outputs inside the steps
M, SEED = 3, 41
EG = _lib.FLAG_ENSEMBLE_GRAD if hasattr(_lib, 'FLAG_ENSEMBLE_GRAD') else 256


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('ensemble-gradient GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


class _launches:
    """Records (members, forward kernel, flag bit) of every SolveCall launched inside the block and (members, adjoint kernel) of
    every call a backward entry point ran on, each read from the call's own descriptor."""

    def __enter__(self):
        self.seen, self.rev = [], []
        self._saved = (engine.SolveCall.launch, engine.solve_backward, engine.backward_with_gradients)
        launch, solve_backward, bwg, rec = *self._saved, self

        def launch_(call, *a, **k):
            rec.seen.append((int(call.desc.members), engine.forward_kernel(call), bool(int(call.base_flags) & EG)))
            return launch(call, *a, **k)

        def solve_backward_(call, *a, **k):
            rec.rev.append((int(call.desc.members), engine.backward_kernel(call)))
            return solve_backward(call, *a, **k)

        def bwg_(call, *a, **k):
            rec.rev.append((int(call.desc.members), engine.backward_kernel(call)))
            return bwg(call, *a, **k)
        engine.SolveCall.launch, engine.solve_backward, engine.backward_with_gradients = launch_, solve_backward_, bwg_
        return self

    def __exit__(self, *exc):
        engine.SolveCall.launch, engine.solve_backward, engine.backward_with_gradients = self._saved
        return False


_MEMBERS = {}


def _members(io, no, H, C_=3, Bm=8, NL=2):
    """M modules of one architecture with DIFFERENT random parameters (requiring grad) on one control path, and the initial states."""
    key = (io, no, H, C_, Bm, NL)
    if key not in _MEMBERS:
        pr = make_problem(300 + H + C_ + Bm, io, no, NL, Bm, H, C_, len(TIMES), times=TIMES)
        coeffs, times = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)
        sdes = []
        for m in range(M):
            torch.manual_seed(1000 + 17 * m + H)
            sde = S.Diffusion_model(C_, H, H, NL, input_option=io, noise_option=no).to(DEV)
            sde.set_X(coeffs, times)
            sdes.append(sde)
        y0 = (0.5 * torch.randn(M, Bm, H, generator=torch.Generator().manual_seed(7 + H))).to(DEV)
        _MEMBERS[key] = (sdes, y0, engine.model_struct(C_, H, H, NL, io, no))
    sdes, y0, model = _MEMBERS[key]
    for sde in sdes:
        sde.requires_grad_(True)
        sde.zero_grad(set_to_none=True)
    return sdes, y0, model


def _take_grads(sdes):
    out = [{n: (None if p.grad is None else p.grad.clone()) for n, p in sde.named_parameters()} for sde in sdes]
    for sde in sdes:
        sde.zero_grad(set_to_none=True)
    return out


def _cotangent(shape, only=None, row_out=False):
    cot = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    if only is not None:      # non-zero on one member only
        mask = torch.zeros(M, device=DEV)
        mask[only] = 1.0
        cot = cot * (mask.reshape(M, 1, 1) if row_out else mask.reshape(1, M, 1, 1))
    return cot


def _ensemble(sdes, y0, method, opts, fwd, rev, only=None):
    """One fused training solve + backward; asserts the route on the launched descriptor.  Returns (ys, dL/dy0, grads, cotangent)."""
    ts = torch.from_numpy(TS).to(DEV)
    ya = y0.clone().requires_grad_(True)
    with _launches() as rec:
        got = S.sdeint_ensemble(sdes, ya, ts, method=method, dt=1.0, options=dict(opts, ensemble_grad=True, strict=True))
        assert type(got.grad_fn).__name__ != 'StackBackward0'
        cot = _cotangent(got.shape, only, 'row_out' in opts)
        (got * cot).sum().backward()
    assert rec.seen == [(M, fwd, True)], rec.seen      # ONE forward launch, of the ensemble descriptor with the flag, on the kernel meant
    assert rec.rev == [(M, rev)], rec.rev              # ... and one adjoint over all members
    return got.detach(), ya.grad, _take_grads(sdes), cot


def _shards(sdes, y0, method, opts, fwd, rev, cot, Bm, row_offset, G, members=range(M)):
    """The members one after the other as shards of the whole, under the same cotangent."""
    ts = torch.from_numpy(TS).to(DEV)
    out = {}
    with _launches() as rec:
        for m in members:
            ym = y0[m].clone().requires_grad_(True)
            ref = S.sdeint(sdes[m], ym, ts, method=method, dt=1.0, options=dict(opts, row_offset=row_offset + m * Bm, global_rows=G, strict=True))
            (ref * (cot[m] if 'row_out' in opts else cot[:, m])).sum().backward()
            out[m] = (ref.detach(), ym.grad)
    n = len(list(members))
    assert rec.seen == [(0, fwd, False)] * n and rec.rev == [(0, rev)] * n, (rec.seen, rec.rev)      # (the kernels the ensemble ran)
    grads = _take_grads(sdes)
    return {m: out[m] + (grads[m],) for m in members}


def _check(io, no, H, C_=3, Bm=8, NL=2, method='euler', kernel='auto', exact_order=False, row_out=False, row_offset=0, global_rows=None,
           param_pass=None, fwd='lean', rev='general', only=None):
    sdes, y0, model = _members(io, no, H, C_, Bm, NL)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    assert grid.N == 8
    G = global_rows or M * Bm
    # the route, on the descriptor the training launch will carry
    q = dict(method=method, kernel=kernel, global_rows=G, row_offset=row_offset, exact_order=exact_order, members=M, ensemble_grad=True,
             training=True)
    desc = engine.query_descriptor(model, M * Bm, len(TIMES), grid.N, **q)
    assert int(desc.flags) & EG
    assert_kernels(desc, fwd=fwd, rev=rev)
    assert engine.backward_mode(model, M * Bm, len(TIMES), grid, method, kernel, exact_order, global_rows=G, members=M, ensemble_grad=True) == 1
    opts = {'seed': SEED, 'kernel': kernel, 'exact_order': exact_order}
    if param_pass:
        opts['param_pass'] = param_pass
    if row_out:
        opts['row_out'] = torch.randint(0, len(TS), (Bm,), generator=torch.Generator().manual_seed(3)).to(DEV)
    eopts = dict(opts, row_offset=row_offset, global_rows=global_rows)
    got, gy0, grads, cot = _ensemble(sdes, y0, method, eopts, fwd, rev, only)
    assert tuple(got.shape) == ((M, Bm, H) if row_out else (len(TS), M, Bm, H)) and torch.isfinite(got).all()
    refs = _shards(sdes, y0, method, opts, fwd, rev, cot, Bm, row_offset, G)
    for m in range(M):
        ys_m, gy_m, gp_m = refs[m]
        mine = got[m] if row_out else got[:, m]
        assert torch.equal(mine, ys_m), (m, 'ys', float((mine - ys_m).abs().max()))
        assert torch.equal(gy0[m], gy_m), (m, 'y0.grad', float((gy0[m] - gy_m).abs().max()))
        for name, g in grads[m].items():
            assert (g is None) == (gp_m[name] is None), (m, name)
            if g is not None:
                assert torch.equal(g, gp_m[name]), (m, name, float((g - gp_m[name]).abs().max()), float(gp_m[name].abs().max()))
    if only is None:
        assert all(float(gy0[m].abs().max()) > 0 and float(grads[m]['linear_out.weight'].abs().max()) > 0 for m in range(M))
    return got, gy0, grads


# ---- 1. bit identity against the members as shards ------------------------------------------------------------------------------

@pytest.mark.parametrize('method', ['euler', 'milstein'])
@pytest.mark.parametrize('H', [64, 128])
def test_lean_kernel_and_the_general_adjoint(H, method):
    _check(4, 17, H, method=method)


def test_mfma4_under_euler_on_the_lean_and_on_the_general_forward():
    _check(4, 17, 64, kernel='mfma4')
    _check(4, 17, 128, kernel='mfma4', exact_order=True, fwd='general_m4')      # (the unfused emb order: the general kernel's)


def test_srk_on_the_general_kernel_and_its_srk_adjoint():
    _check(4, 17, 64, method='srk', fwd='general_m4', rev='general_srk')


def test_time_free_embedded_drift_at_h32():
    _check(2, 16, 32, NL=1)


def test_y_dependent_diffusion_leaves_theta_partials_without_a_table():
    _check(4, 8, 64)


@pytest.mark.parametrize('no', [3, 5, 13])
def test_closed_form_and_one_layer_table_diffusions(no):
    """noise_option 3 / 5: exp(sigma) y and exp(sigma_diag) t - the sigma reduction after the epilogue; 13: the one-layer noise MLP."""
    _check(4, no, 64)


def test_row_out_and_a_shard_of_a_larger_problem():
    _check(4, 17, 64, row_out=True)
    _check(4, 17, 64, method='srk', row_out=True, fwd='general_m4', rev='general_srk')
    _check(4, 17, 64, row_offset=24, global_rows=96)


def test_one_tile_per_member():
    _check(4, 17, 64, Bm=4)


def test_split_parameter_pass_writes_every_adjoint():
    a = _check(4, 17, 64, param_pass='split')
    b = _check(4, 17, 64)
    assert torch.equal(a[1], b[1]) and all(torch.equal(a[2][m][n], b[2][m][n]) for m in range(M) for n in a[2][m])


def test_kept_increments_instead_of_regenerated_ones(monkeypatch):
    b = _check(4, 17, 64)
    monkeypatch.setenv('SNSDE_KEEP_INCREMENTS', '1')
    a = _check(4, 17, 64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][m][n], b[2][m][n]) for m in range(M) for n in a[2][m])


# ---- 2. isolation ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('method,fwd,rev', [('euler', 'lean', 'general'), ('srk', 'general_m4', 'general_srk')])
def test_a_cotangent_on_one_member_reaches_that_member_only(method, fwd, rev):
    got, gy0, grads = _check(4, 17, 64, method=method, fwd=fwd, rev=rev, only=1)
    for m in (0, 2):
        assert int(torch.count_nonzero(gy0[m])) == 0
        for name, g in grads[m].items():
            assert g is not None and int(torch.count_nonzero(g)) == 0, (m, name)
    assert float(gy0[1].abs().max()) > 0 and float(grads[1]['linear_out.weight'].abs().max()) > 0


# ---- 3. members share nothing but the control path ------------------------------------------------------------------------------

def test_members_share_nothing_but_the_control_path():
    """The same initial state and (noise_option 0) no diffusion: the members' gradients still part, and each equals its shard's."""
    sdes, y0, model = _members(4, 0, 64)
    same = y0[:1].expand(M, -1, -1).contiguous()
    got, gy0, grads, cot = _ensemble(sdes, same, 'euler', {'seed': SEED}, 'lean', 'general')
    refs = _shards(sdes, same, 'euler', {'seed': SEED}, 'lean', 'general', cot, 8, 0, 24)
    w = 'linear_out.weight'
    assert (grads[0][w] - grads[1][w]).abs().max() > 1e-3 and (grads[1][w] - grads[2][w]).abs().max() > 1e-3
    for m in range(M):
        assert torch.equal(got[:, m], refs[m][0]) and torch.equal(gy0[m], refs[m][1])
        assert all(torch.equal(g, refs[m][2][n]) for n, g in grads[m].items())


# ---- 4. independent of the single-model route: the engine against the fp64 tensor-op loop ---------------------------------------

T2 = np.array([0.0, 0.6, 1.7, 2.2, 3.9, 4.4, 6.0], np.float32)      # (tests/test_gpu_sample_grad.py)
TS2 = np.array([0.0, 2.5, 6.0], np.float32)


class _ReplayBM:
    def __init__(self, dW, dU=None):
        self.dW, self.dU, self.n = dW, dU, 0

    def __call__(self, ta, tb, return_U=False):
        out = self.dW[self.n]
        u = self.dU[self.n] if self.dU is not None else None
        self.n += 1
        return (out, u) if return_U else out


@pytest.mark.parametrize('io,no,H,C_,NL,dt', [(4, 17, 128, 21, 2, 0.5), (2, 16, 32, 3, 1, 1.0)])
@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_engine_ensemble_against_the_fp64_loop(io, no, H, C_, NL, dt, method):
    """SolveCall(members = 3, ensemble_grad) + backward_with_gradients on supplied increments against the fp64 tensor-op loop of
    every member on its slice, at the project's gradient yardstick 1e-4 (tests/test_gpu_parity.py)."""
    Bm = 8
    rng = np.random.default_rng(77 + H)
    pr = make_problem(610 + H, io, no, NL, Bm, H, C_, len(T2), times=T2)
    grid = engine.step_grid(TS2, dt, T2, torch.device(DEV))
    hh = (grid.t1 - grid.t0).astype(np.float32).reshape(-1, 1, 1)
    y0 = (0.5 * rng.standard_normal((M, Bm, H))).astype(np.float32)
    dW = (rng.standard_normal((grid.N, M * Bm, H)).astype(np.float32) * np.sqrt(hh)).astype(np.float32)
    dU = None
    if method == 'srk':
        dU = (hh * (0.5 * dW + np.sqrt(hh / 12) * rng.standard_normal(dW.shape).astype(np.float32))).astype(np.float32)
    cot = rng.standard_normal((len(TS2), M * Bm, H)).astype(np.float32)
    sdes = []
    for m in range(M):
        torch.manual_seed(2000 + m + H)
        sdes.append(S.Diffusion_model(C_, H, H, NL, input_option=io, noise_option=no))
    model, layout, numel = None, None, None
    coeffs = torch.from_numpy(pr['coeffs']).to(DEV)
    flats = []
    for sde in sdes:
        sde.set_X(torch.from_numpy(pr['coeffs']), torch.from_numpy(T2))
        model, layout, numel = engine.recognise(sde)
        flats.append(engine.flatten_params(sde, layout, numel, torch.device(DEV)))
    flat = torch.stack(flats).contiguous()
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV).contiguous()
    call = engine.SolveCall(model, flat, coeffs, grid, dev(y0.reshape(M * Bm, H)), dW=dev(dW), dU=dev(dU), method=method, save_traj=True,
                            save_dW=method == 'srk', save_act=True, members=M, ensemble_grad=True)
    assert int(call.desc.members) == M and int(call.base_flags) & EG
    assert_kernels(call, fwd='general_m4' if method == 'srk' else 'lean', rev='general_srk' if method == 'srk' else 'general')
    ys = call.launch()
    adj, grad = engine.backward_with_gradients(call, dev(cot), adj0_only=True)
    torch.cuda.synchronize()
    assert tuple(grad.shape) == (M, numel)
    for m in range(M):
        rows = slice(m * Bm, (m + 1) * Bm)
        ref = S.Diffusion_model(C_, H, H, NL, input_option=io, noise_option=no).double()
        ref.load_state_dict({k: v.double() for k, v in sdes[m].state_dict().items()})
        ref.set_X(torch.from_numpy(pr['coeffs']).double(), torch.from_numpy(T2))
        y0r = torch.from_numpy(y0[m]).double().requires_grad_(True)
        bm = _ReplayBM(torch.from_numpy(dW[:, rows]).double(), None if dU is None else torch.from_numpy(dU[:, rows]).double())
        yr = S.sdeint(ref, y0r, torch.from_numpy(TS2), bm=bm, method=method, dt=dt, options={'backend': 'torch'})
        (yr * torch.from_numpy(cot[:, rows]).double()).sum().backward()
        tag = f'({io},{no}) H={H} {method} member {m}'
        assert_parity(ys[:, rows].cpu().numpy(), yr.detach().numpy(), what=tag)
        grad_close(adj[0][rows], y0r.grad, 'y0', 1e-4, tag)
        mine = engine.param_index(sdes[m], layout).grads_from_flat(grad[m])
        for (name, p), g in zip(ref.named_parameters(), mine):
            if p.grad is None or float(p.grad.abs().max()) == 0.0:
                assert float(g.abs().max()) < 1e-6, (tag, name)
                continue
            grad_close(g, p.grad, name, 1e-4, tag)


# ---- 5. the front end -----------------------------------------------------------------------------------------------------------

def _wrappers(kind, H=64, C_=3, Bm=8):
    pr = make_problem(77, 4, 17, 2, Bm, H, C_, len(TIMES), times=TIMES)
    models = []
    for m in range(M):
        torch.manual_seed(500 + m)
        func = S.Diffusion_model(C_, H, H, 2, input_option=4, noise_option=17)
        models.append(kind(func, C_, H, 5).to(DEV).train().requires_grad_(True))
    return models, torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)


@pytest.mark.parametrize('kind,fwd,rev', [(S.NeuralSDE, 'lean', 'general'), (S.IstsNeuralSDE, 'general_m4', 'general_srk')])
def test_ensemble_module_trains_like_the_wrappers(kind, fwd, rev):
    models, coeffs, times = _wrappers(kind)
    fi = torch.tensor([8, 3, 5, 2, 8, 1, 0, 6], device=DEV)
    args = (coeffs, times) if kind is S.IstsNeuralSDE else (times, (coeffs,), fi)
    first = (lambda o: o[0]) if kind is S.IstsNeuralSDE else (lambda o: o)
    ens = S.Ensemble(models).train()
    torch.manual_seed(9)      # (the classification head's Dropout draws per member, in member order in both arms)
    with _launches() as rec:
        got = first(ens(*args, options={'seed': SEED, 'ensemble_grad': True}))
        cot = torch.randn(got.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
        (got * cot).sum().backward()
    assert rec.seen == [(M, fwd, True)] and rec.rev == [(M, rev)], (rec.seen, rec.rev)
    mine = [{n: p.grad.clone() for n, p in net.named_parameters()} for net in models]
    for net in models:
        net.zero_grad(set_to_none=True)
    torch.manual_seed(9)
    with _launches() as ref_rec:
        refs = torch.stack([first(net(*args, options={'seed': SEED, 'row_offset': 8 * m, 'global_rows': 8 * M})) for m, net in enumerate(models)])
        (refs * cot).sum().backward()
    assert ref_rec.seen == [(0, fwd, False)] * M and ref_rec.rev == [(0, rev)] * M
    assert torch.equal(got, refs)
    for gm, net in zip(mine, models):
        for n, p in net.named_parameters():
            assert torch.equal(gm[n], p.grad), (n, float((gm[n] - p.grad).abs().max()))
        assert float(gm['func.linear_out.weight'].abs().max()) > 0 and float(gm['initial_network.weight'].abs().max()) > 0
    with pytest.raises(ValueError, match='inference only'):
        ens(*args, options={'seed': SEED})


def test_uncovered_plan_loops_and_strict_raises():
    """noise_option 18 at H = 64 is the wave pairs' plan and H = 256 the two-tile kernels': no ensemble adjoint, so the M
    differentiable solves run and are stacked; strict raises; without the opt-in the parent's ValueError stays."""
    ts = torch.from_numpy(TS).to(DEV)
    for (io, no, H), fwd in (((1, 18, 64), 'w4'), ((4, 17, 256), None)):
        sdes, y0, model = _members(io, no, H)
        grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
        assert engine.backward_mode(model, M * 8, len(TIMES), grid, 'euler', global_rows=M * 8, members=M, ensemble_grad=True) == 0
        ya = y0.clone().requires_grad_(True)
        with _launches() as rec:
            got = S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0, options={'seed': SEED, 'ensemble_grad': True})
            cot = _cotangent(got.shape)
            (got * cot).sum().backward()
        assert [s[0] for s in rec.seen] == [0] * M and (fwd is None or [s[1] for s in rec.seen] == [fwd] * M), rec.seen
        grads = _take_grads(sdes)
        yb = y0.clone().requires_grad_(True)
        ref = torch.stack([S.sdeint(sdes[m], yb[m], ts, method='euler', dt=1.0,
                                    options={'seed': SEED, 'row_offset': 8 * m, 'global_rows': M * 8}) for m in range(M)], dim=1)
        (ref * cot).sum().backward()
        assert torch.equal(got, ref) and torch.equal(ya.grad, yb.grad)
        for gm, gr in zip(grads, _take_grads(sdes)):
            assert all(torch.equal(gm[n], gr[n]) for n in gm)
        with pytest.raises(NotImplementedError, match='strict'):
            S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0, options={'seed': SEED, 'ensemble_grad': True, 'strict': True})
        with pytest.raises(ValueError, match='inference only'):
            S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0, options={'seed': SEED})


# ---- 6. entry-point equivalence -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_backward_with_gradients_equals_the_two_calls(method):
    sdes, y0, model = _members(4, 17, 64)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    flat = torch.stack([engine.flatten_params(sde, *engine.recognise(sde)[1:], torch.device(DEV)) for sde in sdes])
    call = engine.SolveCall(model, flat, sdes[0].coeffs, grid, y0.reshape(M * 8, 64).contiguous(), method=method, seed=SEED,
                            save_traj=True, save_dW=method == 'srk', save_act=True, members=M, ensemble_grad=True)
    ys = call.launch()
    cot = torch.randn(ys.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    adj, grad = engine.backward_with_gradients(call, cot, adj0_only=True)
    adj, grad = adj.clone(), grad.clone()
    for adj0_only in (True, False):
        adj2, delta = engine.solve_backward(call, cot, save_delta=True, adj0_only=adj0_only)
        grad2 = engine.param_gradients(call, adj2, delta)
        torch.cuda.synchronize()
        assert torch.equal(adj[0], adj2[0]) and torch.equal(grad, grad2) and tuple(grad.shape) == (M, flat.shape[1])
    assert float(grad.abs().max()) > 0
