"""Training through wave-pair model ensembles on the GPU: options={'ensemble_nets': True, 'ensemble_grad': True,
'ensemble_nets_grad': True} (SNSDE_FLAG_ENSEMBLE_NETS | SNSDE_FLAG_ENSEMBLE_GRAD | SNSDE_FLAG_ENSEMBLE_NETS_GRAD) against the ordinary
differentiable sdeint of each member run as a shard of the whole (members = 0, its own parameters, row_offset + m Bm, the same
global_rows) - states, dL/dy0 and every parameter gradient member by member, torch.equal, no tolerance: the ENS instantiations of
the training forward (snsde_w4_euler_kernel / snsde_w4_srk_kernel), of the two adjoints (snsde_w4_euler_reverse_kernel,
snsde_w4_srk_reverse_kernel) and the two reduction kernels carry the member on a grid axis and run every sum in the member's own
order.  Every case first asserts, on the descriptors actually launched, that ONE forward launch with members = M ran on 'w4' with
the three flag bits set and ONE backward on 'w4_fused', and that the member-alone references ran the same kernels with members = 0:
the loop of M solves cannot stand in silently.

Shapes (H = 64, C = 3, nine irregular knots, eight steps of dt = 1 - two Philox blocks -, outputs between the steps, a fixed seed):
M = 3 members of Bm = 8 rows (one workgroup of two pairs each) for every instantiation; Bm = 4 (one tile: the workgroup's second
pair is a dead surplus pair), Bm = 12 (an odd tile count: the surplus pair of a member's last workgroup is that member's), Bm = 68
(17 tiles, nsplit = 16, per = 2: nine splits hold tiles, seven are empty) and M = 2 x Bm = 260 (65 tiles, per = 5: the four-way
unrolled body of the first reduce stage and its remainder)."""
import copy
import signal

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests.helpers import assert_kernels, make_problem

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

TIMES = np.array([0.0, 0.6, 1.7, 2.2, 3.9, 4.4, 6.0, 6.9, 8.0], np.float32)      # L = 9 knots
TS = np.array([0.0, 2.5, 5.3, 8.0], np.float32)                                  # outputs inside the steps
SEED, H, C_ = 41, 64, 3
ALL = 2048 | 1024 | 256      # SNSDE_FLAG_ENSEMBLE_NETS_GRAD | SNSDE_FLAG_ENSEMBLE_NETS | SNSDE_FLAG_ENSEMBLE_GRAD
THREE = {'ensemble_nets': True, 'ensemble_grad': True, 'ensemble_nets_grad': True}


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
    """Records (members, forward kernel, the three flag bits all set) of every SolveCall launched inside the block and (members,
    adjoint kernel) of every call a backward entry point ran on, each read from the call's own descriptor."""

    def __enter__(self):
        self.seen, self.rev = [], []
        self._saved = (engine.SolveCall.launch, engine.solve_backward, engine.backward_with_gradients)
        launch, solve_backward, bwg, rec = *self._saved, self

        def launch_(call, *a, **k):
            rec.seen.append((int(call.desc.members), engine.forward_kernel(call), int(call.base_flags) & ALL == ALL))
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


def _members(io, no, NL=2, Bm=8, M=3):
    """M modules of one architecture with DIFFERENT random parameters (requiring grad) on one control path, and the initial states."""
    key = (io, no, NL, Bm, M)
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


def _ensemble(sdes, y0, method, opts):
    """One fused training solve + backward; asserts the route on the launched descriptors.  Returns (ys, dL/dy0, grads, cotangent)."""
    M = len(sdes)
    ts = torch.from_numpy(TS).to(DEV)
    ya = y0.clone().requires_grad_(True)
    with _launches() as rec:
        got = S.sdeint_ensemble(sdes, ya, ts, method=method, dt=1.0, options=dict(opts, strict=True, **THREE))
        assert type(got.grad_fn).__name__ != 'StackBackward0'
        cot = torch.randn(got.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
        (got * cot).sum().backward()
    assert rec.seen == [(M, 'w4', True)], rec.seen      # ONE forward launch of the ensemble descriptor with the three bits, on the pairs
    assert rec.rev == [(M, 'w4_fused')], rec.rev        # ... and one adjoint over all members
    return got.detach(), ya.grad, _take_grads(sdes), cot


def _shards(sdes, y0, method, opts, cot, Bm, row_offset, G):
    """The members one after the other as shards of the whole, under the same cotangent."""
    M = len(sdes)
    ts = torch.from_numpy(TS).to(DEV)
    out = {}
    with _launches() as rec:
        for m in range(M):
            ym = y0[m].clone().requires_grad_(True)
            ref = S.sdeint(sdes[m], ym, ts, method=method, dt=1.0, options=dict(opts, row_offset=row_offset + m * Bm, global_rows=G, strict=True))
            (ref * (cot[m] if 'row_out' in opts else cot[:, m])).sum().backward()
            out[m] = (ref.detach(), ym.grad)
    assert rec.seen == [(0, 'w4', False)] * M and rec.rev == [(0, 'w4_fused')] * M, (rec.seen, rec.rev)      # (the kernels the ensemble ran)
    grads = _take_grads(sdes)
    return {m: out[m] + (grads[m],) for m in range(M)}


def _check(io, no, NL=2, Bm=8, M=3, method='euler', row_out=False, row_offset=0, global_rows=None, param_pass=None, seed=SEED):
    sdes, y0, model = _members(io, no, NL, Bm, M)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    assert grid.N == 8
    G = global_rows or M * Bm
    # the route, on the descriptor the training launch will carry
    q = dict(method=method, global_rows=G, row_offset=row_offset, members=M, training=True, **THREE)
    desc = engine.query_descriptor(model, M * Bm, len(TIMES), grid.N, **q)
    assert int(desc.flags) & ALL == ALL
    assert_kernels(desc, fwd='w4', rev='w4_fused')
    assert engine.backward_mode(model, M * Bm, len(TIMES), grid, method, global_rows=G, members=M, **THREE) == 1
    assert engine.backward_mode(model, M * Bm, len(TIMES), grid, method, global_rows=G, members=M, ensemble_grad=True, ensemble_nets=True) == 0
    opts = {'seed': seed}
    if param_pass:
        opts['param_pass'] = param_pass
    if row_out:
        opts['row_out'] = torch.randint(0, len(TS), (Bm,), generator=torch.Generator().manual_seed(3)).to(DEV)
    got, gy0, grads, cot = _ensemble(sdes, y0, method, dict(opts, row_offset=row_offset, global_rows=global_rows))
    assert tuple(got.shape) == ((M, Bm, H) if row_out else (len(TS), M, Bm, H)) and torch.isfinite(got).all()
    refs = _shards(sdes, y0, method, opts, cot, Bm, row_offset, G)
    for m in range(M):
        ys_m, gy_m, gp_m = refs[m]
        mine = got[m] if row_out else got[:, m]
        assert torch.equal(mine, ys_m), (m, 'ys', float((mine - ys_m).abs().max()))
        assert torch.equal(gy0[m], gy_m), (m, 'y0.grad', float((gy0[m] - gy_m).abs().max()))
        for name, g in grads[m].items():
            assert (g is None) == (gp_m[name] is None), (m, name)
            if g is not None:
                assert torch.equal(g, gp_m[name]), (m, name, float((g - gp_m[name]).abs().max()), float(gp_m[name].abs().max()))
    # non-zero, and the members' own
    net_w = 'noise_y.0.weight' if no >= 18 else 'noise_y.weight'
    for m in range(M):
        assert float(gy0[m].abs().max()) > 0, m
        for name in ('linear_in.weight', 'linear_out.weight', 'linear_out.bias', net_w, 'theta'):
            assert grads[m][name] is not None and float(grads[m][name].abs().max()) > 0, (m, name)
    for m in range(1, M):
        assert (grads[m]['linear_out.weight'] - grads[0]['linear_out.weight']).abs().max() > 0
        assert (grads[m][net_w] - grads[0][net_w]).abs().max() > 0
    return got, gy0, grads


# ---- 1. every ENS instantiation, Bm = 8 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('io', [1, 5])
@pytest.mark.parametrize('no', [14, 15, 18, 19])
@pytest.mark.parametrize('NL', [1, 2])
def test_srk_every_adjoint_instantiation(NL, no, io):
    """CfgSR<NHID, NN, GEO, MULY>: NL - 1 hidden drift layers x one- / two-layer net x the gated drift x raw = q * state."""
    _check(io, no, NL, method='srk')


@pytest.mark.parametrize('NL,no', [(1, 15), (2, 18)])
def test_srk_time_feature_forward(NL, no):
    _check(3, no, NL, method='srk')


@pytest.mark.parametrize('io', [1, 3])
@pytest.mark.parametrize('no', [14, 18])
@pytest.mark.parametrize('NL', [1, 2])
def test_euler_every_training_forward_instantiation(NL, no, io):
    """CfgW<NHID, NN, TIME, SAVE = true>, ENS and the four fused Euler adjoints CfgW<NHID, NN>."""
    _check(io, no, NL)


@pytest.mark.parametrize('NL,no', [(1, 19), (2, 15)])
def test_euler_gated_drift_and_state_multiplied_net(NL, no):
    _check(5, no, NL)


# ---- 2. tiles per member -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_one_tile_per_member_has_a_dead_surplus_pair(method):
    """Bm = 4: tiles_m = 1, nsplit = 1; the second pair of every workgroup must write no block and add nothing to theta."""
    _check(1, 18, Bm=4, method=method)


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_odd_tile_count_keeps_the_surplus_pair_in_its_member(method):
    _check(3, 19, Bm=12, method=method)


def test_seventeen_tiles_split_sixteen_ways():
    """Bm = 68: per = 2 - the first nine splits hold tiles, the other seven are empty."""
    _check(1, 18, Bm=68)


def test_sixty_five_tiles_unrolled_body_and_remainder():
    """M = 2, Bm = 260: per = 5 - one pass of the four-way unrolled body and a remainder tile in every split, per member."""
    _check(1, 18, Bm=260, M=2)


# ---- 3. what stays per global row --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_row_out(method):
    _check(3, 18, method=method, row_out=True)


def test_every_adjoint_written_equals_dl_dy0_only():
    """The front end's default asks for dL/dy0 only (SNSDE_BWD_ADJ0_ONLY, one call); param_pass='split' writes every a_n and takes
    the two calls: the same gradients, and both equal the members' own."""
    for method in ('euler', 'srk'):
        a = _check(1, 18, method=method)
        b = _check(1, 18, method=method, param_pass='split')
        assert torch.equal(a[1], b[1]) and all(torch.equal(a[2][m][n], b[2][m][n]) for m in range(3) for n in a[2][m])


def test_a_shard_of_a_larger_problem():
    _check(1, 18, row_offset=24, global_rows=96)
    _check(1, 18, method='srk', row_offset=24, global_rows=96)


def test_device_resident_seed_reads_the_forwards_increments():
    """A one-element CUDA tensor as the Philox key (the graph-replay form): the Euler adjoint cannot regenerate from it and reads
    the increments the forward left in dW_out - for the right global rows; the same bits as under the host key."""
    key = torch.tensor([SEED], dtype=torch.int64, device=DEV)
    a = _check(1, 18, seed=key)
    b = _check(1, 18)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][m][n], b[2][m][n]) for m in range(3) for n in a[2][m])


# ---- 4. the front end --------------------------------------------------------------------------------------------------------------

def test_strict_does_not_raise_on_the_fused_route_and_raises_off_it():
    sdes, y0, model = _members(1, 18)
    ts = torch.from_numpy(TS).to(DEV)
    ya = y0.clone().requires_grad_(True)
    with _launches() as rec:
        S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0, options=dict(THREE, seed=SEED, strict=True)).sum().backward()
    assert rec.seen == [(3, 'w4', True)] and rec.rev == [(3, 'w4_fused')]
    _take_grads(sdes)
    for opts in ({'ensemble_nets': True, 'ensemble_grad': True}, {'ensemble_grad': True}):      # (the M differentiable solves: strict raises)
        with pytest.raises(NotImplementedError, match='strict'):
            S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0, options=dict(opts, seed=SEED, strict=True))
    with pytest.raises(NotImplementedError, match='strict'):      # Milstein through the net: the diffusion-net tiles, no ensemble adjoint
        S.sdeint_ensemble(sdes, ya, ts, method='milstein', dt=1.0, options=dict(THREE, seed=SEED, strict=True))


@pytest.mark.filterwarnings('ignore:sdeint. no fused gradient')
def test_coefficients_that_require_grad_take_the_loop_route():
    sdes, y0, model = _members(1, 18)
    ts = torch.from_numpy(TS).to(DEV)
    shared = sdes[0].coeffs
    coeffs = shared.detach().clone().requires_grad_(True)
    times = torch.from_numpy(TIMES).to(DEV)
    try:
        for sde in sdes:
            sde.set_X(coeffs, times)
        ya = y0.clone().requires_grad_(True)
        with _launches() as rec:
            got = S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0, options=dict(THREE, seed=SEED))
            cot = torch.randn(got.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
            (got * cot).sum().backward()
        # the loop route: the members' own differentiable solves, nothing with members = M.  (Each of them is what sdeint does for
        # one such model whose coefficients require grad: the pair adjoint leaves no delta planes for dL/dcoeffs, so it differentiates
        # through the tensor-op loop and launches no fused solve at all - hence "none with members = M", not "M with members = 0")
        assert all(s[0] == 0 for s in rec.seen) and all(r[0] == 0 for r in rec.rev), (rec.seen, rec.rev)
        assert type(got.grad_fn).__name__ == 'StackBackward0'
        grads = _take_grads(sdes)
        yb = y0.clone().requires_grad_(True)
        ref = torch.stack([S.sdeint(sdes[m], yb[m], ts, method='euler', dt=1.0,
                                    options={'seed': SEED, 'row_offset': 8 * m, 'global_rows': 24}) for m in range(3)], dim=1)
        (ref * cot).sum().backward()
        assert torch.equal(got, ref) and torch.equal(ya.grad, yb.grad)
        for gm, gr in zip(grads, _take_grads(sdes)):
            assert all(torch.equal(gm[n], gr[n]) for n in gm if gm[n] is not None)
        with pytest.raises(NotImplementedError, match='strict'):
            S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0, options=dict(THREE, seed=SEED, strict=True))
    finally:
        for sde in sdes:
            sde.set_X(shared, times)


def test_ensemble_module_trains_two_steps_like_the_members_trained_separately():
    """Ensemble([...]).train() with the three options: one fused forward and one fused backward per optimizer step; after two SGD
    steps on its loss every parameter equals that of the M wrappers trained separately at their row offsets."""
    M, Bm = 3, 8
    pr = make_problem(77, 1, 18, 2, Bm, H, C_, len(TIMES), times=TIMES)
    coeffs, times = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)
    models = []
    for m in range(M):
        torch.manual_seed(500 + m)
        func = S.Diffusion_model(C_, H, H, 2, input_option=1, noise_option=18)
        models.append(S.NeuralSDE(func, C_, H, 5).to(DEV).train().requires_grad_(True))
    alone = copy.deepcopy(models)
    start = models[0].func.linear_out.weight.detach().clone()
    fi = torch.tensor([8, 3, 5, 2, 8, 1, 0, 6], device=DEV)
    ens = S.Ensemble(models).train()
    opt = torch.optim.SGD(ens.parameters(), lr=0.05)
    opts_alone = [torch.optim.SGD(net.parameters(), lr=0.05) for net in alone]
    cot = None
    losses, losses_alone = [], []
    torch.manual_seed(9)      # (the classification head's Dropout draws per member, in member order in both arms)
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        with _launches() as rec:
            got = ens(times, (coeffs,), fi, options=dict(THREE, seed=SEED + step))
            if cot is None:
                cot = torch.randn(got.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
            loss = (got * cot).sum()
            loss.backward()
        assert rec.seen == [(M, 'w4', True)] and rec.rev == [(M, 'w4_fused')], (step, rec.seen, rec.rev)
        opt.step()
        losses.append(loss.detach())
    torch.manual_seed(9)
    for step in range(2):
        with _launches() as rec:
            outs = []
            for m, net in enumerate(alone):
                opts_alone[m].zero_grad(set_to_none=True)
                outs.append(net(times, (coeffs,), fi, options={'seed': SEED + step, 'row_offset': Bm * m, 'global_rows': Bm * M}))
            loss = (torch.stack(outs) * cot).sum()
            loss.backward()
        assert rec.seen == [(0, 'w4', False)] * M and rec.rev == [(0, 'w4_fused')] * M, (step, rec.seen, rec.rev)
        for o in opts_alone:
            o.step()
        losses_alone.append(loss.detach())
    assert all(torch.equal(a, b) for a, b in zip(losses, losses_alone))
    for net, ref in zip(models, alone):
        for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
            assert torch.equal(p, q), (n, float((p - q).abs().max()))
    assert float((models[0].func.linear_out.weight.detach() - start).abs().max()) > 0      # (the steps moved the parameters)
