"""Sample paths of a model ensemble on the GPU: members = M = 3 models x samples = S paths per input row in ONE fused solve
(options={'samples': S, 'ensemble_samples': True}, SNSDE_FLAG_ENSEMBLE_SAMPLES) against the SAMPLED sdeint of each member run as
a shard of the whole (members = 0, samples = S, its own parameters, row_offset + m Bm, the same global_rows) - member by member,
torch.equal, no tolerance - for every kernel that takes both options, and the same for training (states, dL/dy0, every parameter
gradient) under the three opt-ins together.  Every case first asserts, on the descriptor it launches, that the fused route is taken
and which kernel it names, and counts the launches: the loop of M sampled solves cannot stand in silently.

Shapes: those of tests/test_gpu_ensemble.py - nine irregular knots, eight steps of dt = 1 that cross every spline interval, output
times inside the steps, Philox under a fixed seed, C = 3.  S = 3 on 4 input rows: Bm = 12 paths per member is three 4-row tiles,
and every tile straddles two input rows (its coefficient rows are not one row repeated); S = 2 on 2 input rows is one tile per
member; S = 5 on 4 input rows has tiles inside one input row and tiles across two."""
import signal

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests.helpers import make_problem

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

TIMES = np.array([0.0, 0.6, 1.7, 2.2, 3.9, 4.4, 6.0, 6.9, 8.0], np.float32)      # L = 9 knots
TS = np.array([0.0, 2.5, 5.3, 8.0], np.float32)                                  # outputs inside the steps
M, SEED = 3, 41
ES = 512      # SNSDE_FLAG_ENSEMBLE_SAMPLES


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('ensemble-samples GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


class _launches:
    """Records (members, samples, forward kernel, flag bit) of every SolveCall launched inside the block and (members, samples,
    adjoint kernel) of every call a backward entry point ran on, each read from the call's own descriptor."""

    def __enter__(self):
        self.seen, self.rev = [], []
        self._saved = (engine.SolveCall.launch, engine.solve_backward, engine.backward_with_gradients)
        launch, solve_backward, bwg, rec = *self._saved, self

        def launch_(call, *a, **k):
            rec.seen.append((int(call.desc.members), int(call.desc.samples), engine.forward_kernel(call), bool(int(call.base_flags) & ES)))
            return launch(call, *a, **k)

        def solve_backward_(call, *a, **k):
            rec.rev.append((int(call.desc.members), int(call.desc.samples), engine.backward_kernel(call)))
            return solve_backward(call, *a, **k)

        def bwg_(call, *a, **k):
            rec.rev.append((int(call.desc.members), int(call.desc.samples), engine.backward_kernel(call)))
            return bwg(call, *a, **k)
        engine.SolveCall.launch, engine.solve_backward, engine.backward_with_gradients = launch_, solve_backward_, bwg_
        return self

    def __exit__(self, *exc):
        engine.SolveCall.launch, engine.solve_backward, engine.backward_with_gradients = self._saved
        return False


_MEMBERS = {}


def _members(io, no, H, C_=3, rows=4, Sn=3, NL=2, grad=False):
    """M modules of one architecture with DIFFERENT random parameters on one control path of `rows` input rows, and the members'
    initial states, one per PATH (M, rows Sn, H): the paths of an input row start apart as well."""
    key = (io, no, H, C_, rows, Sn, NL)
    if key not in _MEMBERS:
        pr = make_problem(300 + H + C_ + rows, io, no, NL, rows, H, C_, len(TIMES), times=TIMES)
        coeffs, times = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)
        sdes = []
        for m in range(M):
            torch.manual_seed(1000 + 17 * m + H)
            sde = S.Diffusion_model(C_, H, H, NL, input_option=io, noise_option=no).to(DEV)
            sde.set_X(coeffs, times)
            sdes.append(sde)
        y0 = (0.5 * torch.randn(M, rows * Sn, H, generator=torch.Generator().manual_seed(7 + H))).to(DEV)
        _MEMBERS[key] = (sdes, y0, engine.model_struct(C_, H, H, NL, io, no))
    sdes, y0, model = _MEMBERS[key]
    for sde in sdes:
        sde.requires_grad_(grad)
        sde.zero_grad(set_to_none=True)
    return sdes, y0, model


def _check(io, no, H, C_=3, rows=4, Sn=3, method='euler', kernel='auto', precision='fp32', lean_general=False, exact_order=False,
           row_out=False, row_offset=0, global_rows=None, expect=None, variant=None, replicated=False):
    """The fused sampled ensemble against its members' sampled solves as shards; returns the ensemble's result."""
    sdes, y0, model = _members(io, no, H, C_, rows, Sn)
    Bm = rows * Sn
    ts = torch.from_numpy(TS).to(DEV)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    assert grid.N == 8
    G = global_rows or M * Bm
    # the route, on the descriptor the launch will carry
    q = dict(method=method, kernel=kernel, precision=precision, global_rows=G, row_offset=row_offset, lean_general=lean_general,
             exact_order=exact_order, members=M, samples=Sn, ensemble_samples=True)
    assert engine.forward_path(model, M * Bm, len(TIMES), grid.N, **q) != 'none'
    assert engine.forward_path(model, M * Bm, len(TIMES), grid.N, **dict(q, ensemble_samples=False)) == 'none'
    desc = engine.query_descriptor(model, M * Bm, len(TIMES), grid.N, **q)
    assert engine.forward_kernel(desc) == expect, (engine.forward_kernel(desc, keys=True), 'meant', expect)
    if variant is not None:
        assert engine.lean_variant(desc) == variant
    opts = {'seed': SEED, 'kernel': kernel, 'precision': precision, 'exact_order': exact_order, 'samples': Sn}
    if row_out:      # one entry per PATH: the paths of an input row are read at different output times
        opts['row_out'] = torch.randint(0, len(TS), (Bm,), generator=torch.Generator().manual_seed(3)).to(DEV)
    with _launches() as rec, torch.no_grad():
        got = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=1.0,
                                options=dict(opts, ensemble_samples=True, row_offset=row_offset, global_rows=global_rows,
                                             lean_general=lean_general, strict=True))
    assert rec.seen == [(M, Sn, expect, True)], rec.seen      # ONE launch with members = M and samples = S, on the kernel meant
    assert tuple(got.shape) == ((M, Bm, H) if row_out else (len(TS), M, Bm, H))
    assert torch.isfinite(got).all()
    with _launches() as ref_rec, torch.no_grad():
        for m in range(M):
            ref = S.sdeint(sdes[m], y0[m], ts, method=method, dt=1.0, options=dict(opts, row_offset=row_offset + m * Bm, global_rows=G))
            mine = got[m] if row_out else got[:, m]
            assert torch.equal(mine, ref), (m, float((mine - ref).abs().max()))
    assert ref_rec.seen == [(0, Sn, expect, False)] * M, ref_rec.seen      # (the sampled shards ran the kernel the ensemble ran)
    if replicated:      # ... and the members' ordinary solves on hand-replicated coefficients
        coeffs, times = sdes[0].coeffs, sdes[0].times
        try:
            with torch.no_grad():
                for m in range(M):
                    sdes[m].set_X(coeffs.repeat_interleave(Sn, dim=0), times)
                    ref = S.sdeint(sdes[m], y0[m], ts, method=method, dt=1.0,
                                   options=dict({k: v for k, v in opts.items() if k != 'samples'}, row_offset=row_offset + m * Bm, global_rows=G))
                    assert torch.equal(got[m] if row_out else got[:, m], ref), m
        finally:
            for sde in sdes:
                sde.set_X(coeffs, times)
    if not row_out:
        last = got[-1].reshape(M, rows, Sn, H)
        assert (last[1] - last[0]).abs().max() > 1e-3 and (last[2] - last[1]).abs().max() > 1e-3      # the members differ
        assert (last[:, :, 1] - last[:, :, 0]).abs().max() > 1e-3                                      # the paths of an input row differ
    return got


# ---- 1. inference: bit identity against the members' sampled solves -----------------------------------------------------------

@pytest.mark.parametrize('method', ['euler', 'milstein'])
@pytest.mark.parametrize('H', [64, 128])
def test_lean_general_kernel(H, method):
    _check(4, 17, H, method=method, lean_general=True, expect='lean', variant='general', replicated=(H == 64 and method == 'euler'))


def test_lean_specialised_kernel():
    spec = _check(4, 17, 128, C_=21, expect='lean', variant='specialised')
    gen = _check(4, 17, 128, C_=21, lean_general=True, expect='lean', variant='general')
    assert torch.equal(spec, gen)


def test_lean_kernel_with_bf16_operands():
    bf = _check(4, 17, 128, precision='bf16', expect='lean_bf16')
    f32 = _check(4, 17, 128, expect='lean')
    assert 0 < (bf - f32).abs().max() < 0.25      # (another kernel than the f32 one, and still the same solve: states are O(1))


def test_general_kernel_under_euler_and_under_srk():
    _check(4, 17, 128, kernel='mfma4', exact_order=True, expect='general_m4', replicated=True)
    _check(4, 17, 128, kernel='mfma4', method='srk', expect='general_m4')
    _check(4, 17, 64, method='srk', expect='general_m4')


def test_one_tile_per_member_and_five_paths_per_row():
    _check(4, 17, 64, rows=2, Sn=2, lean_general=True, expect='lean')                 # Bm = 4
    _check(4, 17, 64, rows=4, Sn=5, lean_general=True, expect='lean')                 # Bm = 20
    _check(4, 17, 64, rows=4, Sn=5, method='srk', expect='general_m4')


def test_row_out_and_a_shard_of_a_larger_problem():
    _check(4, 17, 64, row_out=True, lean_general=True, expect='lean')
    _check(4, 17, 128, method='srk', row_out=True, expect='general_m4')
    _check(4, 17, 64, row_offset=42, global_rows=120, lean_general=True, expect='lean')
    _check(4, 17, 128, method='srk', row_offset=24, global_rows=72, expect='general_m4')


def test_initial_states_and_row_out_per_input_row_are_expanded():
    sdes, y0, model = _members(4, 17, 64)
    ts = torch.from_numpy(TS).to(DEV)
    per_row = y0[:, ::3].contiguous()      # (M, 4, H)
    ro = torch.tensor([3, 0, 2, 1], device=DEV)
    opts = {'seed': SEED, 'samples': 3, 'ensemble_samples': True, 'strict': True}
    with _launches() as rec, torch.no_grad():
        a = S.sdeint_ensemble(sdes, per_row, ts, method='euler', dt=1.0, options=opts)
        b = S.sdeint_ensemble(sdes, per_row.repeat_interleave(3, dim=1), ts, method='euler', dt=1.0, options=opts)
        c = S.sdeint_ensemble(sdes, per_row, ts, method='euler', dt=1.0, options=dict(opts, row_out=ro))
    assert rec.seen == [(M, 3, 'lean', True)] * 3
    assert tuple(a.shape) == (len(TS), M, 12, 64) and torch.equal(a, b)
    idx = ro.repeat_interleave(3).reshape(1, 1, -1, 1).expand(1, M, 12, 64)
    assert tuple(c.shape) == (M, 12, 64) and torch.equal(c, a.gather(0, idx).squeeze(0))
    with torch.no_grad():
        for m in range(M):
            assert torch.equal(a[:, m], S.sdeint(sdes[m], per_row[m], ts, method='euler', dt=1.0,
                                                 options={'seed': SEED, 'samples': 3, 'row_offset': 12 * m, 'global_rows': 36}))


def test_uncovered_plan_loops_and_strict_raises():
    """noise_option 18 at H = 64 under `auto` is the wave pairs' plan: no kernel maps its rows to members, so sdeint_ensemble runs
    the M sampled solves and raises under strict; without the opt-in samples > 1 raises as before."""
    sdes, y0, model = _members(1, 18, 64)
    ts = torch.from_numpy(TS).to(DEV)
    assert engine.forward_path(model, M * 12, len(TIMES), 8, 'euler', members=M, samples=3, ensemble_samples=True, global_rows=M * 12) == 'none'
    opts = {'seed': SEED, 'samples': 3, 'ensemble_samples': True}
    with _launches() as rec, torch.no_grad():
        got = S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=1.0, options=opts)
    assert len(rec.seen) == M and all(s[0] == 0 for s in rec.seen), rec.seen
    with torch.no_grad():
        ref = torch.stack([S.sdeint(sdes[m], y0[m], ts, method='euler', dt=1.0,
                                    options={'seed': SEED, 'samples': 3, 'row_offset': 12 * m, 'global_rows': M * 12}) for m in range(M)], dim=1)
        assert torch.equal(got, ref)
        with pytest.raises(NotImplementedError, match='strict'):
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=1.0, options=dict(opts, strict=True))
        with pytest.raises(ValueError, match='samples'):
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=1.0, options={'seed': SEED, 'samples': 3})


# ---- 2. training ----------------------------------------------------------------------------------------------------------------

def _take_grads(sdes):
    out = [{n: (None if p.grad is None else p.grad.clone()) for n, p in sde.named_parameters()} for sde in sdes]
    for sde in sdes:
        sde.zero_grad(set_to_none=True)
    return out


TRAIN = {'ensemble_samples': True, 'ensemble_grad': True, 'sample_grad': True}


def _check_training(H, method, fwd, rev, rows=4, Sn=3, only=None, kernel='auto', row_offset=0, global_rows=None):
    sdes, y0, model = _members(4, 17, H, 3, rows, Sn, grad=True)
    Bm = rows * Sn
    ts = torch.from_numpy(TS).to(DEV)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    G = global_rows or M * Bm
    q = dict(members=M, samples=Sn, ensemble_samples=True, ensemble_grad=True, sample_grad=True)
    assert engine.backward_mode(model, M * Bm, len(TIMES), grid, method, kernel, global_rows=G, **q) == 1
    desc = engine.query_descriptor(model, M * Bm, len(TIMES), grid.N, method=method, kernel=kernel, global_rows=G, row_offset=row_offset,
                                   training=True, **q)
    assert engine.forward_kernel(desc) == fwd and engine.backward_kernel(desc) == rev
    opts = {'seed': SEED, 'kernel': kernel, 'samples': Sn}
    ya = y0.clone().requires_grad_(True)
    with _launches() as rec:
        got = S.sdeint_ensemble(sdes, ya, ts, method=method, dt=1.0,
                                options=dict(opts, row_offset=row_offset, global_rows=global_rows, strict=True, **TRAIN))
        assert type(got.grad_fn).__name__ != 'StackBackward0'
        cot = torch.randn(got.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
        if only is not None:      # non-zero on one member's paths only
            mask = torch.zeros(M, device=DEV)
            mask[only] = 1.0
            cot = cot * mask.reshape(1, M, 1, 1)
        (got * cot).sum().backward()
    assert rec.seen == [(M, Sn, fwd, True)], rec.seen      # ONE forward launch ...
    assert rec.rev == [(M, Sn, rev)], rec.rev              # ... and ONE backward launch over all members and paths
    got, gy0, grads = got.detach(), ya.grad, _take_grads(sdes)
    assert tuple(got.shape) == (len(TS), M, Bm, H) and torch.isfinite(got).all()
    with _launches() as ref_rec:
        for m in range(M):
            ym = y0[m].clone().requires_grad_(True)
            ref = S.sdeint(sdes[m], ym, ts, method=method, dt=1.0,
                           options=dict(opts, sample_grad=True, row_offset=row_offset + m * Bm, global_rows=G, strict=True))
            (ref * cot[:, m]).sum().backward()
            gp = _take_grads(sdes)[m]
            assert torch.equal(got[:, m], ref.detach()), (m, 'ys', float((got[:, m] - ref).abs().max()))
            assert torch.equal(gy0[m], ym.grad), (m, 'y0.grad', float((gy0[m] - ym.grad).abs().max()))
            for name, g in grads[m].items():
                assert (g is None) == (gp[name] is None), (m, name)
                if g is not None:
                    assert torch.equal(g, gp[name]), (m, name, float((g - gp[name]).abs().max()), float(gp[name].abs().max()))
    assert ref_rec.seen == [(0, Sn, fwd, False)] * M and ref_rec.rev == [(0, Sn, rev)] * M, (ref_rec.seen, ref_rec.rev)
    if only is None:
        assert all(float(gy0[m].abs().max()) > 0 and float(grads[m]['linear_out.weight'].abs().max()) > 0 for m in range(M))
    for sde in sdes:
        sde.requires_grad_(False)
    return got, gy0, grads


@pytest.mark.parametrize('method,fwd,rev', [('euler', 'lean', 'general'), ('srk', 'general_m4', 'general_srk')])
def test_training_equals_the_members_sampled_solves(method, fwd, rev):
    _check_training(64, method, fwd, rev)


def test_training_at_h128_one_tile_per_member_and_a_shard():
    _check_training(128, 'euler', 'lean', 'general')
    _check_training(64, 'euler', 'lean', 'general', rows=2, Sn=2)
    _check_training(64, 'euler', 'lean', 'general', row_offset=24, global_rows=96)
    _check_training(64, 'milstein', 'lean', 'general', rows=4, Sn=5)


@pytest.mark.parametrize('method,fwd,rev', [('euler', 'lean', 'general'), ('srk', 'general_m4', 'general_srk')])
def test_a_cotangent_on_one_members_paths_reaches_that_member_only(method, fwd, rev):
    got, gy0, grads = _check_training(64, method, fwd, rev, only=1)
    for m in (0, 2):
        assert int(torch.count_nonzero(gy0[m])) == 0
        for name, g in grads[m].items():
            assert g is not None and int(torch.count_nonzero(g)) == 0, (m, name)
    assert float(gy0[1].abs().max()) > 0 and float(grads[1]['linear_out.weight'].abs().max()) > 0


def test_coefficients_that_require_grad_take_the_loop_and_give_the_summed_gradient():
    sdes, y0, model = _members(4, 17, 64, grad=True)
    ts = torch.from_numpy(TS).to(DEV)
    base, times = sdes[0].coeffs, sdes[0].times
    opts = {'seed': SEED, 'samples': 3}
    try:
        c = base.clone().requires_grad_(True)
        for sde in sdes:
            sde.set_X(c, times)
        with _launches() as rec:
            got = S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=1.0, options=dict(opts, **TRAIN))
            got.sum().backward()
        assert [s[:2] for s in rec.seen] == [(0, 3)] * M, rec.seen      # the M sampled differentiable solves
        with pytest.raises(NotImplementedError, match='strict'):
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=1.0, options=dict(opts, strict=True, **TRAIN))
        c2 = base.clone().requires_grad_(True)
        for sde in sdes:
            sde.set_X(c2, times)
        ref = torch.stack([S.sdeint(sdes[m], y0[m], ts, method='euler', dt=1.0,
                                    options=dict(opts, sample_grad=True, row_offset=12 * m, global_rows=36)) for m in range(M)], dim=1)
        ref.sum().backward()
        assert torch.equal(got, ref)
        assert tuple(c.grad.shape) == tuple(base.shape) and c.grad.abs().max() > 0 and torch.equal(c.grad, c2.grad)
        # ... which is the sum of the members' own (each already summed over its S paths), in autograd's order of the M additions
        total = mag = None
        for m in range(M):
            cm = base.clone().requires_grad_(True)
            sdes[m].set_X(cm, times)
            S.sdeint(sdes[m], y0[m], ts, method='euler', dt=1.0,
                     options=dict(opts, sample_grad=True, row_offset=12 * m, global_rows=36)).sum().backward()
            total = cm.grad if total is None else total + cm.grad
            mag = cm.grad.abs() if mag is None else mag + cm.grad.abs()
        # (M - 1 = 2 float32 additions per element, in one order here and possibly another there: each sum is within
        #  2 u sum|terms| of the exact one, u = 2^-24, so the two are within 4 u sum|terms| of each other; 5 u for the rounding of `mag`)
        assert ((c.grad - total).abs() <= 5 * 2.0 ** -24 * mag).all()
    finally:
        for sde in sdes:
            sde.set_X(base, times)
            sde.zero_grad(set_to_none=True)
            sde.requires_grad_(False)


def test_strict_raises_on_an_uncovered_training_plan_and_the_opt_ins_are_needed():
    sdes, y0, model = _members(1, 18, 64, grad=True)      # a diffusion net: no ensemble adjoint
    ts = torch.from_numpy(TS).to(DEV)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    assert engine.backward_mode(model, M * 12, len(TIMES), grid, 'euler', 'mfma4', members=M, samples=3, ensemble_samples=True,
                                ensemble_grad=True, sample_grad=True) == 0
    ya = y0.clone().requires_grad_(True)
    opts = {'seed': SEED, 'samples': 3, 'kernel': 'mfma4'}
    try:
        with pytest.raises(NotImplementedError, match='strict'):
            S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0, options=dict(opts, strict=True, **TRAIN))
        with pytest.raises(ValueError, match='sample_grad'):
            S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0, options=dict(opts, ensemble_samples=True, ensemble_grad=True))
        with pytest.raises(ValueError, match='inference only'):
            S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0, options=dict(opts, ensemble_samples=True, sample_grad=True))
    finally:
        for sde in sdes:
            sde.requires_grad_(False)


# ---- 3. the Ensemble wrapper ----------------------------------------------------------------------------------------------------

def test_ensemble_of_classification_wrappers_with_sample_paths():
    pr = make_problem(77, 4, 17, 2, 4, 64, 3, len(TIMES), times=TIMES)
    models = []
    for m in range(M):
        torch.manual_seed(500 + m)
        func = S.Diffusion_model(3, 64, 64, 2, input_option=4, noise_option=17)
        net = S.NeuralSDE(func, 3, 64, 5).to(DEV)
        for mod in net.linear:
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.normal_(); mod.running_var.uniform_(0.5, 2.0)
        models.append(net.eval().requires_grad_(False))
    coeffs, times = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)
    fi = torch.tensor([8, 3, 5, 1], device=DEV)
    ens = S.Ensemble(models).eval()
    with _launches() as rec, torch.no_grad():
        got = ens(times, (coeffs,), fi, options={'seed': SEED, 'samples': 3, 'ensemble_samples': True})
    assert rec.seen == [(M, 3, 'lean', True)], rec.seen
    with _launches() as ref_rec, torch.no_grad():
        refs = [net(times, (coeffs,), fi, options={'seed': SEED, 'samples': 3, 'row_offset': 12 * m, 'global_rows': 12 * M})
                for m, net in enumerate(models)]
    assert ref_rec.seen == [(0, 3, 'lean', False)] * M
    assert tuple(got.shape) == (M, 12, 5) and torch.isfinite(got).all()
    assert torch.equal(got, torch.stack(refs))
    assert (got[0] - got[1]).abs().max() > 1e-4
    mean, within, between = S.ensemble_stats(got, M, 3)      # the stacked (M, B S, out) readout: outer = 1
    assert tuple(mean.shape) == (4, 5) and (within > 0).all() and (between > 0).all()
