"""Particle filtering on sample paths on the host: the entry point snsde_sample_resample (declared, exported, bound, validating
before it launches), engine.sample_resample_tensor_ops - the tensor-op statement of the definition - in float64 against
hand-checkable answers and the numpy statement of tests/sample_resample_reference.py, the properties of systematic resampling, the
special values, engine.filter_paths against a by-hand trace, and torchsde.sdeint_filter on CPU tensors.  No GPU compute.

Bounds: the statement runs in float64 here, so the comparisons use the bounds of the reference with unit = 8 x 2^-53 (torch's
sums and logsumexp take another order than the kernel's chain; a handful of roundings each)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests import sample_resample_reference as R
from tests.test_step_offset_cpu import Stub, _model

ERR_NULL, ERR_DIMS = -1, -2
INF, NAN = float('inf'), float('nan')
UNIT = 8 * R.U64


def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'snsde.h')).read()
    lib = _lib.lib()
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    name = 'snsde_sample_resample'
    assert f'SNSDE_API int {name}(' in header
    assert name in _lib.EXPORTS and hasattr(lib, name)
    assert f' T {name}\n' in dyn
    assert len(getattr(lib, name).argtypes) == 16
    assert lib.snsde_version() == 2      # (an entry point added, no struct changed)
    assert S.sample_resample is engine.sample_resample and S.filter_paths is engine.filter_paths
    assert S.sdeint_filter is S.torchsde.sdeint_filter
    assert S.torchsde.sample_resample is engine.sample_resample and S.torchsde.filter_paths is engine.filter_paths


def _call(lib, groups=1, samples=4, width=3, stratified=0, threshold=0.5, state=4096, logw=8192, loginc=0, u=12288, state_out=1 << 30,
          logw_out=1 << 31, ancestor=1 << 32, ess=1 << 33, logz=1 << 34, resampled=1 << 35):
    """Dummy non-null pointers: every case here must be refused before anything is launched."""
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_resample(p(state), p(logw), p(loginc), p(u), groups, samples, width, stratified, threshold, p(state_out),
                                     p(logw_out), p(ancestor), p(ess), p(logz), p(resampled), None)


def test_the_entry_point_validates_before_it_launches():
    lib = _lib.lib()
    for name in ('state', 'logw', 'u', 'state_out', 'logw_out', 'ancestor', 'ess', 'logz', 'resampled'):
        assert _call(lib, **{name: 0}) == ERR_NULL, name
    assert _call(lib, samples=0) == ERR_DIMS and _call(lib, samples=257) == ERR_DIMS and _call(lib, width=0) == ERR_DIMS
    assert _call(lib, groups=0) == ERR_DIMS and _call(lib, groups=-3) == ERR_DIMS and _call(lib, samples=-1) == ERR_DIMS
    assert _call(lib, threshold=NAN) == ERR_DIMS
    assert _call(lib, groups=2 ** 61, width=8) == ERR_DIMS and _call(lib, groups=2 ** 62, samples=1, width=1) == ERR_DIMS      # 63 bits
    # state_out overlapping state: the same pointer, one float in, one float before the end - and the first byte past it is not
    nbytes = 1 * 4 * 3 * 4
    for off in (0, 4, nbytes - 4, -4, -(nbytes - 4)):
        assert _call(lib, state=1 << 20, state_out=(1 << 20) + off) == ERR_DIMS, off
    assert _call(lib, state=0, samples=257) == ERR_NULL      # (pointers first, as the siblings)


def _run(w, u, threshold=1.0, stratified=False, inc=None, state=None, log=True):
    """The statement on weights w (G, S) given as plain (log=True) or log weights, in float64."""
    w = torch.as_tensor(w, dtype=torch.float64)
    G, Sn = w.shape
    lw = w.log() if log else w
    x = torch.arange(G * Sn, dtype=torch.float64).reshape(G * Sn, 1) if state is None else state
    return engine.sample_resample_tensor_ops(x, Sn, lw, inc, torch.as_tensor(u, dtype=torch.float64), threshold, stratified)


def test_hand_checked_answers():
    out = _run([[0.1, 0.2, 0.3, 0.4]], [0.5])
    assert out.ancestor.tolist() == [[1, 2, 3, 3]] and out.ancestor.dtype == torch.int32 and out.resampled.tolist() == [1]
    assert abs(float(out.ess) - 1 / 0.3) <= 1e-12 and abs(float(out.logz) - math.log(0.25)) <= 1e-12
    assert out.state[:, 0].tolist() == [1.0, 2.0, 3.0, 3.0]
    assert torch.equal(out.log_weight, out.logz[:, None].expand(1, 4))
    # unnormalised weights: the same ancestors, the evidence moves
    big = _run([[10., 20., 30., 40.]], [0.5])
    assert big.ancestor.tolist() == [[1, 2, 3, 3]] and abs(float(big.logz) - math.log(25.0)) <= 1e-12
    # uniform weights give the identity for any u (t_j = j + u)
    for u in (0.0, 0.25, 0.5, 0.875):
        assert _run(torch.ones(2, 5), [u, u]).ancestor.tolist() == [[0, 1, 2, 3, 4]] * 2
    # one live particle is the ancestor of all
    one = _run([[0.0, 0.0, 3.0, 0.0]], [0.3])
    assert one.ancestor.tolist() == [[2, 2, 2, 2]] and abs(float(one.ess) - 1.0) <= 1e-15 and abs(float(one.logz) - math.log(0.75)) <= 1e-12
    # the increment adds to the carried weight
    inc = _run([[0.1, 0.1, 0.1, 0.1]], [0.5], inc=torch.tensor([[0.1, 0.2, 0.3, 0.4]], dtype=torch.float64).log())
    assert inc.ancestor.tolist() == [[1, 2, 3, 3]] and abs(float(inc.logz) - math.log(0.025)) <= 1e-12
    # S = 1: the identity, ess = 1
    s1 = _run([[0.3], [2.0]], [0.9, 0.1])
    assert s1.ancestor.tolist() == [[0], [0]] and s1.ess.tolist() == [1.0, 1.0] and torch.allclose(s1.logz, torch.tensor([0.3, 2.0], dtype=torch.float64).log())


@pytest.mark.parametrize('stratified', [False, True])
@pytest.mark.parametrize('scale', R.SCALES)
@pytest.mark.parametrize('shape', [(3, 2, 5), (5, 7, 33), (2, 64, 8), (4, 256, 4), (2, 255, 3), (301, 4, 3)], ids=str)
def test_the_statement_against_the_numpy_reference(shape, scale, stratified):
    G, Sn, W = shape
    c = R.make_case(shape, scale)
    f64 = lambda k: torch.from_numpy(c[k].astype(np.float64))
    u = c['us'] if stratified else c['u']
    for inc in (None, c['loginc']):
        for threshold in R.THRESHOLDS:
            ref = R.reference(c['logw'].astype(np.float64), None if inc is None else inc.astype(np.float64), u, threshold, stratified, unit=UNIT)
            out = engine.sample_resample_tensor_ops(f64('state').reshape(G * Sn, W), Sn, f64('logw'), None if inc is None else f64('loginc'),
                                                    torch.from_numpy(u.astype(np.float64)), threshold, stratified)
            assert tuple(out.state.shape) == (G * Sn, W) and tuple(out.ancestor.shape) == (G, Sn) and tuple(out.ess.shape) == (G,)
            got = dict(ancestor=out.ancestor.numpy().astype(np.int64), ess=out.ess.numpy(), logz=out.logz.numpy(),
                       resampled=out.resampled.numpy().astype(np.int64), logw_out=out.log_weight.numpy())
            assert R.check_outputs(ref, got, threshold, Sn, f'{shape} {scale} {threshold}') == 0      # (float64: no comparison is that close)
            want = f64('state')[torch.arange(G)[:, None], out.ancestor.long()].reshape(G * Sn, W)
            assert torch.equal(out.state, want)
            assert torch.equal(engine.sample_resample(f64('state').reshape(G * Sn, W), Sn, f64('logw'), None if inc is None else f64('loginc'),
                                                      torch.from_numpy(u.astype(np.float64)), threshold, stratified).ancestor, out.ancestor)
            lse = torch.logsumexp(out.log_weight, dim=-1) - math.log(Sn)      # the evidence is carried in the weights, either way
            assert float((lse - out.logz).abs().max()) <= 64 * Sn * R.U64 * (1 + float(out.logz.abs().max()))


def test_systematic_resampling_is_monotone_with_floor_or_ceil_offspring():
    gen = torch.Generator().manual_seed(11)
    G, Sn = 64, 37
    lw = 2.0 * torch.randn(G, Sn, generator=gen, dtype=torch.float64)
    out = engine.sample_resample_tensor_ops(torch.zeros(G * Sn, 1, dtype=torch.float64), Sn, lw, None, torch.rand(G, generator=gen, dtype=torch.float64), 1.0)
    anc = out.ancestor.long()
    assert bool((anc[:, 1:] >= anc[:, :-1]).all())
    w = torch.softmax(lw, dim=-1) * Sn
    counts = torch.zeros(G, Sn, dtype=torch.float64).scatter_add_(1, anc, torch.ones(G, Sn, dtype=torch.float64))
    assert bool(((counts >= torch.floor(w - 1e-9)) & (counts <= torch.ceil(w + 1e-9))).all()) and bool((counts.sum(1) == Sn).all())


def test_stratified_resampling_reads_one_uniform_per_path():
    w = [[0.1, 0.2, 0.3, 0.4]]
    # t_j = (j + u_j) / 4 against P / P_3 = (0.1, 0.3, 0.6, 1): u = (0.5, 0.1, 0.5, 0.1) -> t = (0.125, 0.275, 0.625, 0.775)
    assert _run(w, [[0.5, 0.1, 0.5, 0.1]], stratified=True).ancestor.tolist() == [[1, 1, 3, 3]]
    assert _run(w, [[0.3, 0.3, 0.3, 0.9]], stratified=True).ancestor.tolist() == [[0, 2, 2, 3]]
    same = torch.full((1, 4), 0.5, dtype=torch.float64)
    assert torch.equal(_run(w, same, stratified=True).ancestor, _run(w, [0.5]).ancestor)
    with pytest.raises(ValueError, match='u has shape'):
        _run(w, [0.5], stratified=True)
    with pytest.raises(ValueError, match='u has shape'):
        _run(w, same)


def test_threshold_semantics():
    w = [[0.1, 0.2, 0.3, 0.4], [0.25, 0.25, 0.25, 0.25], [0.97, 0.01, 0.01, 0.01]]      # ess = 3.33, 4, 1.06
    u = [0.5, 0.5, 0.5]
    for threshold, want in ((0.0, [0, 0, 0]), (-1.0, [0, 0, 0]), (0.5, [0, 0, 1]), (0.9, [1, 0, 1]), (1.0, [1, 1, 1]), (7.0, [1, 1, 1])):
        out = _run(w, u, threshold)
        assert out.resampled.tolist() == want, threshold
        lw = torch.tensor(w, dtype=torch.float64).log()
        for g, r in enumerate(want):
            if r:
                assert torch.equal(out.log_weight[g], out.logz[g].expand(4))
            else:
                assert out.ancestor[g].tolist() == [0, 1, 2, 3] and torch.equal(out.log_weight[g], lw[g])
                assert out.state[4 * g:4 * g + 4, 0].tolist() == [4.0 * g + k for k in range(4)]
    for bad in (NAN, None, 'half', True):
        with pytest.raises(ValueError, match='threshold'):
            _run(w, u, bad)


# ---- special values (the table tests/test_gpu_sample_resample.py runs on the device) --------------------------------------------------------

BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))      # the largest float32 below 1


def special_cases():
    """name -> (log-weights (G, 4), u (G), what the row must come out as).  Row 1 is the special one, rows 0 and 2 are ordinary."""
    ordinary = [0.3, -0.2, 0.1, -1.0]
    return {
        'a -Inf weight is never an ancestor': ([ordinary, [-INF, 0.0, -INF, 0.5], ordinary], [0.1, 0.999, 0.1], 'live'),
        'far below the maximum is never an ancestor': ([ordinary, [-300.0, 0.0, -250.0, 0.5], ordinary], [0.1, 0.0, 0.1], 'live'),
        'dead trailing particles and u just below 1': ([ordinary, [0.2, 0.0, -INF, -INF], ordinary], [0.1, BELOW_ONE, 0.1], 'live'),
        'dead leading particles and u = 0': ([ordinary, [-INF, -INF, 0.0, 0.2], ordinary], [0.1, 0.0, 0.1], 'live'),
        'all -Inf': ([ordinary, [-INF] * 4, ordinary], [0.1, 0.5, 0.1], 'dead'),
        'a NaN': ([ordinary, [0.1, NAN, 0.2, 0.0], ordinary], [0.1, 0.5, 0.1], 'nan'),
        'a +Inf': ([ordinary, [0.1, INF, 0.2, 0.0], ordinary], [0.1, 0.5, 0.1], 'nan'),
        'NaN beside -Inf': ([ordinary, [-INF, NAN, -INF, -INF], ordinary], [0.1, 0.5, 0.1], 'nan'),
    }


def special_state(G=3, Sn=4, W=3):
    """A state with NaN, Inf and -0.0 in it: values are only moved."""
    x = torch.arange(G * Sn * W, dtype=torch.float32).reshape(G * Sn, W) + 1
    x[1, 0], x[5, 1], x[6, 2], x[7, 0], x[10, 1] = NAN, INF, -INF, -0.0, NAN
    return x


def check_special(name, out, lw, state, kind, Sn=4):
    """The row-1 rules of a special case on the outputs of `sample_resample` (any device)."""
    lw, anc = lw.cpu(), out.ancestor.cpu().long()
    ess, logz, res, lwo = out.ess.cpu(), out.logz.cpu(), out.resampled.cpu(), out.log_weight.cpu()
    x, xo = state.cpu().reshape(-1, Sn, state.shape[-1]), out.state.cpu().reshape(-1, Sn, state.shape[-1])
    if kind == 'live':
        assert int(res[1]) == 1 and bool(torch.isfinite(logz[1])) and float(ess[1]) > 0, name
        assert bool((torch.exp(lw[1] - lw[1].max())[anc[1]] > 0).all()), (name, anc[1].tolist())
        assert bool((anc[1, 1:] >= anc[1, :-1]).all()), name
    else:
        assert int(res[1]) == 0 and anc[1].tolist() == list(range(Sn)), name
        assert R_bits(lwo[1], lw[1].to(lwo.dtype)), name
        if kind == 'dead':
            assert float(ess[1]) == 0.0 and float(logz[1]) == -INF, name
        else:
            assert bool(torch.isnan(ess[1])) and bool(torch.isnan(logz[1])), name
    for g in (0, 2):      # the neighbours are ordinary
        assert int(res[g]) == 1 and bool(torch.isfinite(ess[g])) and bool(torch.isfinite(logz[g])), name
    moved = x[torch.arange(x.shape[0])[:, None], anc]
    assert R_bits(xo, moved), (name, 'state is moved bit for bit')


def R_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


@pytest.mark.parametrize('name', list(special_cases()))
def test_special_values(name):
    rows, u, kind = special_cases()[name]
    for dtype in (torch.float64, torch.float32):
        lw, state = torch.tensor(rows, dtype=dtype), special_state().to(dtype)
        out = engine.sample_resample(state, 4, lw, None, torch.tensor(u, dtype=dtype), 1.0)      # (CPU: the statement)
        check_special(name, out, lw, state, kind)
    if name == 'dead trailing particles and u just below 1':
        assert out.ancestor[1, -1].item() == 1      # the last live particle, not the clamp at S - 1
    if name == 'dead leading particles and u = 0':
        assert out.ancestor[1, 0].item() == 2


def test_an_input_that_requires_grad_is_a_value_error():
    x, lw, u = torch.zeros(8, 3), torch.zeros(2, 4), torch.full((2,), 0.5)
    for args in ((x.clone().requires_grad_(True), 4, lw), (x, 4, lw.clone().requires_grad_(True)), (x, 4, lw, lw.clone().requires_grad_(True))):
        for fn in (S.sample_resample, engine.sample_resample_tensor_ops):
            with pytest.raises(ValueError, match='inference only.*requires grad'):
                fn(*args, u=u)
            with torch.no_grad():
                assert fn(*args, u=u).ancestor.tolist() == [[0, 1, 2, 3]] * 2
    for bad in (lambda: S.sample_resample(x, 3, lw), lambda: S.sample_resample(x, 4, lw[:1]), lambda: S.sample_resample(x, 4, lw, lw[:, :2]),
                lambda: S.sample_resample(x, 0, lw), lambda: S.sample_resample(x.long(), 4, lw)):
        with pytest.raises(ValueError):
            bad()
    # u=None draws with the generator: reproducible, and uniform weights stay the identity whatever it draws
    w = torch.tensor([[0.1, 0.2, 0.3, 0.4]] * 2).log()
    a = S.sample_resample(x, 4, w, threshold=1.0, generator=torch.Generator().manual_seed(3))
    b = S.sample_resample(x, 4, w, threshold=1.0, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a.ancestor, b.ancestor) and a.resampled.tolist() == [1, 1]
    lead = S.sample_resample(torch.zeros(2, 3, 8, 5), 4, torch.zeros(2, 3, 2, 4), threshold=1.0, stratified=True)      # leading axes fold into groups
    assert tuple(lead.state.shape) == (2, 3, 8, 5) and tuple(lead.ancestor.shape) == (2, 3, 2, 4) and tuple(lead.ess.shape) == (2, 3, 2)


def test_filter_paths_against_a_trace_by_hand():
    T, B, Sn, H = 3, 2, 4, 2
    ys = torch.arange(T * B * Sn * H, dtype=torch.float32).reshape(T, B * Sn, H)
    anc = torch.tensor([[[0, 0, 2, 3], [1, 1, 1, 2]],        # the resampling after ys[0]
                        [[1, 1, 2, 2], [3, 2, 1, 0]],        # ... after ys[1]
                        [[3, 3, 3, 3], [0, 0, 0, 0]]], dtype=torch.int32)      # ... after ys[2]: not used
    out = engine.filter_paths(ys, anc, Sn)
    assert torch.equal(out[2], ys[2])
    # group 0: slots at step 1 = anc[1] = (1, 1, 2, 2); at step 0 = anc[0][(1, 1, 2, 2)] = (0, 0, 2, 2)
    # group 1: slots at step 1 = (3, 2, 1, 0); at step 0 = anc[0][(3, 2, 1, 0)] = (2, 1, 1, 1)
    y = ys.reshape(T, B, Sn, H)
    assert torch.equal(out[1].reshape(B, Sn, H), torch.stack([y[1, 0, [1, 1, 2, 2]], y[1, 1, [3, 2, 1, 0]]]))
    assert torch.equal(out[0].reshape(B, Sn, H), torch.stack([y[0, 0, [0, 0, 2, 2]], y[0, 1, [2, 1, 1, 1]]]))
    ident = torch.arange(Sn, dtype=torch.int32).expand(T, B, Sn)
    assert torch.equal(engine.filter_paths(ys, ident, Sn), ys)
    for bad in (lambda: engine.filter_paths(ys, anc[:2], Sn), lambda: engine.filter_paths(ys, anc.float(), Sn), lambda: engine.filter_paths(ys[0], anc, Sn),
                lambda: engine.filter_paths(ys, anc, 3)):
        with pytest.raises(ValueError):
            bad()


# ---- the driver on CPU tensors (a caller's bm carries the paths) --------------------------------------------------------------------------

TS = torch.tensor([0.0, 0.75, 2.25, 4.0])


def _likelihood(seen):
    def fn(k, yk):
        seen.append((k, yk.clone()))
        return -8.0 * (yk[:, :3] - 0.1 * k).pow(2).sum(-1).reshape(-1, 2)      # (sharp: the weights of two paths differ enough to resample)
    return fn


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_sdeint_filter_on_cpu_tensors(method):
    m, pr = _model()
    y0, Sn = torch.from_numpy(pr['y0']), 2
    options = {'samples': Sn}
    whole = S.sdeint(m, y0, TS, bm=Stub((8, 16)), dt=0.25, method=method, options=dict(options))
    seen = []
    keep = S.sdeint_filter(m, y0, TS, _likelihood(seen), bm=Stub((8, 16)), method=method, dt=0.25, options=options, threshold=0.0)
    assert options == {'samples': Sn} and [k for k, _ in seen] == [1, 2, 3]
    assert torch.equal(keep.ys, whole) and tuple(keep.log_weight.shape) == (4, 4, 2) and tuple(keep.ess.shape) == (4, 4)
    incs = [_likelihood([])(k, whole[k]) for k in (1, 2, 3)]
    run = torch.zeros(4, 2)
    assert torch.equal(keep.log_weight[0], run) and keep.ess[0].tolist() == [2.0] * 4 and keep.logz[0].tolist() == [0.0] * 4
    for k, inc in enumerate(incs, 1):
        run = run + inc
        assert torch.equal(keep.log_weight[k], run)
    assert keep.ancestor.dtype == torch.int32 and torch.equal(keep.ancestor, torch.arange(2, dtype=torch.int32).expand(4, 4, 2))
    # threshold = 1: every piece is the by-hand chain sdeint(.., extra_solver_state) -> sample_resample
    gen = lambda: torch.Generator().manual_seed(5)
    always = S.sdeint_filter(m, y0, TS, _likelihood([]), bm=Stub((8, 16)), method=method, dt=0.25, options=options, threshold=1.0, generator=gen())
    g, y, state, lw = gen(), y0, None, torch.zeros(4, 2)
    for k in (1, 2, 3):
        piece, state = S.sdeint(m, y, TS[k - 1:k + 1], bm=Stub((8, 16)), dt=0.25, method=method, options=dict(options), extra=True,
                                extra_solver_state=state)
        assert torch.equal(always.ys[k], piece[1])
        r = S.sample_resample(piece[1], Sn, lw, _likelihood([])(k, piece[1]), None, 1.0, False, g)
        assert torch.equal(always.ancestor[k], r.ancestor) and torch.equal(always.log_weight[k], r.log_weight) and torch.equal(always.logz[k], r.logz)
        assert r.resampled.tolist() == [1] * 4
        y, lw = r.state, r.log_weight
    assert not torch.equal(always.ys[3], keep.ys[3])      # (it did resample)
    for out in (keep, always):
        lse = torch.logsumexp(out.log_weight[-1], dim=-1) - math.log(Sn)
        assert float((lse - out.logz[-1]).abs().max()) <= 1e-5 * (1 + float(out.logz[-1].abs().max()))
        assert torch.equal(S.filter_paths(out.ys, out.ancestor, Sn)[-1], out.ys[-1])
    with pytest.raises(ValueError, match='samples'):
        S.sdeint_filter(m, y0, TS, _likelihood([]), bm=Stub((8, 16)), method=method, dt=0.25)
    with pytest.raises(ValueError, match='log_likelihood'):
        S.sdeint_filter(m, y0, TS, lambda k, yk: yk, bm=Stub((8, 16)), method=method, dt=0.25, options=options)
    with pytest.raises(NotImplementedError):      # without a bm the tensor-op loop cannot continue a path: sdeint's own refusal, let through
        S.sdeint_filter(m, y0, TS, _likelihood([]), method=method, dt=0.25, options=options)
