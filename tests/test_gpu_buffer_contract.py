"""The stand-alone entry points of include/snsde.h on memory the test controls (tests/buffer_arena.py): every output, workspace
and input of a call sits in an Arena - guard bands on both sides, the whole allocation filled with 0x00, 0xFF or 0x3F - and the
call goes through the C ABI.

How a call is made.  The engine function runs once on ordinary tensors with its C call recorded (`recorded_calls`): the
arguments, the tensor behind every pointer, and which of them the engine allocated - its outputs and workspaces.  `replay` then
makes the SAME call through `_lib.lib().snsde_*` - the same scalars, flags and NULL pointers, so no call shape the suite does not
already run - with every device pointer moved into a fresh arena: inputs copied there, outputs and workspaces holding the fill.

What is asserted, per function, shape, fill and alignment:
  1  return code 0, and every byte outside the views (the guards, the unused rest) still holds the fill;
  2  every input equals the engine's tensor bit for bit;
  3  every output has the same bits under the three fills: an unwritten element keeps its fill, a read-modify-write of an output or
     a read of workspace before it is written differs between them;
  4  the aligned 0x00 result has the bits of what the engine function returned (which the float64 tests of each function hold to
     its reference): no new reference, no tolerance;
  5  snsde_affine_compose / _backward: the union of the jobs' ranges is written and equal across fills, every float outside it still
     holds the fill (include/snsde.h: "the caller zero-fills what no job writes");
  6  the same with every device pointer 4 bytes past a 16-byte boundary: 1 - 3 hold, and the bits equal the aligned ones where
     include/snsde.h promises independence of the pointer alignment (energy, loglik, class); for the others the answer is printed.
The kernels behind these functions read and write global memory one float at a time, except the statistics kernels, whose host
code derives the 16-byte width from the pointers (csrc/snsde_stats.hip); the float4 accesses of the head and energy kernels are to
LDS.  So no function here needs an alignment, and the unaligned arm runs for all of them.

The shapes are the tables of the float64 GPU tests of the same functions (ragged tiles, one column past a chunk, partly empty
packs, grid stride); the inputs are drawn once per shape and finite - but the spline data, where NaN means missing."""
import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine, fields
from tests import sample_class_reference as CR
from tests import score_special_cases as SC
from tests import spline_grad_reference as SG
from tests.buffer_arena import FILLS, Arena, RecordedCall, place, recorded_calls, replay, same_bits
from tests.head_cases import HEAD_KINDS, HEAD_SHAPES, make_head
from tests.helpers import make_problem
from tests.tutorial_fields import COMPOSITION_CASES, TutorialField

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

ALIGNMENT_PROMISED = ('snsde_sample_energy', 'snsde_sample_energy_backward', 'snsde_sample_loglik', 'snsde_sample_loglik_backward',
                      'snsde_sample_class', 'snsde_sample_class_backward')
COMBINATIONS = {'count': 0}         # (function, shape, fill, alignment) combinations run
ALIGNMENT_SEEN = {}                 # function -> [unaligned bits == aligned bits, per call]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rand(rng, *shape):
    return _dev(rng.standard_normal(shape).astype(np.float32))


def _arena(call, fill, extra=()):
    sizes = [t.numel() * t.element_size() for t in call.tensors.values()] + [t.numel() * t.element_size() for t in extra]
    return Arena(DEV, fill, sum(Arena.room(n) for n in sizes) + (1 << 16))


def _sync():
    torch.cuda.current_stream().synchronize()


def hold(call, what):
    """Assertions 1 - 4 and 6 on one recorded call."""
    assert call.rc == 0, (what, call.name, call.rc)
    fn = getattr(_lib.lib(), call.name)
    got = {}
    for offset in (0, 1):
        for fill in FILLS:
            tag = f'{what} {call.name} fill {fill:#04x} offset {offset}'
            arena = _arena(call, fill)
            placed = place(call, arena, offset)
            assert all(p.view.data_ptr() % 16 == 4 * offset for p in placed.values())
            rc = replay(fn, call, placed)
            _sync()
            assert rc == 0, (tag, rc)
            arena.check(tag)
            for p in placed.values():
                if not p.is_output:
                    assert same_bits(p.view, p.original.reshape(-1)), f'{tag}: an input of {p.original.numel()} elements was changed'
            got[offset, fill] = {ptr: p.view.clone() for ptr, p in placed.items() if p.is_output and not p.workspace}
            assert got[offset, fill], f'{tag}: the recording names no output'
            COMBINATIONS['count'] += 1
        for fill in FILLS[1:]:
            for ptr, out in got[offset, fill].items():
                assert same_bits(out, got[offset, 0][ptr]), \
                    f'{what} {call.name} offset {offset}: an output of {out.numel()} elements depends on what its memory held ' \
                    f'(fill {fill:#04x} against 0x00; first at {_first_difference(out, got[offset, 0][ptr])})'
    for ptr, out in got[0, 0].items():
        assert same_bits(out, call.tensors[ptr].reshape(-1)), \
            f'{what} {call.name}: the arena result differs from the engine\'s (first at {_first_difference(out, call.tensors[ptr].reshape(-1))})'
    same = all(same_bits(out, got[0, 0][ptr]) for ptr, out in got[1, 0].items())
    ALIGNMENT_SEEN.setdefault(call.name, []).append(same)
    print(f'{what} {call.name}: unaligned bits == aligned bits: {same}')
    if call.name in ALIGNMENT_PROMISED:
        assert same, f'{what} {call.name}: include/snsde.h promises independence of the pointer alignment'


def _first_difference(a, b):
    d = (a.view(torch.int32) != b.view(torch.int32)).nonzero()
    return int(d[0]) if d.numel() else None


def run(what, thunk, *names):
    with recorded_calls(engine) as rec:
        thunk()
    _sync()
    for name in names:
        hold(rec.named(name), what)


# ---- statistics --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', SC.SHAPES, ids=str)
def test_sample_stats(shape):
    G, N, W = shape
    rng = np.random.default_rng(G + 7 * N + 31 * W)
    ys, gm, gv = _rand(rng, G * N, W), _rand(rng, G, W), _rand(rng, G, W)

    def both():
        mean, var = engine.sample_stats(ys, N, True)
        engine.sample_stats_backward(gm, gv, ys, mean, N)
    run(f'{shape}', both, 'snsde_sample_stats', 'snsde_sample_stats_backward')
    if shape == SC.SHAPES[0]:       # the optional variance absent: var and grad_var NULL, mean not read
        run(f'{shape} mean only', lambda: engine.sample_stats_backward(gm, None, ys, engine.sample_stats(ys, N, False)[0], N),
            'snsde_sample_stats', 'snsde_sample_stats_backward')


@pytest.mark.parametrize('shape', SC.ENSEMBLE_STATS_SHAPES + [SC.ENSEMBLE], ids=str)
def test_ensemble_stats(shape):
    O, M, G, Sn, W = shape
    rng = np.random.default_rng(O + M + G + Sn + W)
    ys = _rand(rng, O, M, G * Sn, W)
    grads = [_rand(rng, O, G, W) for _ in range(3)]

    def both():
        engine.ensemble_stats(ys, M, Sn, True, True)
        engine.ensemble_stats_backward(*grads, ys, M, Sn)
    run(f'{shape}', both, 'snsde_ensemble_stats', 'snsde_ensemble_stats_backward')


# ---- scores ------------------------------------------------------------------------------------------------------------------------

def _pooled_inputs(shape):
    """ys, target, members, samples, lead of a (G, N, W) shape (one member) or the (outer, M, G, S, W) ensemble shape."""
    rng = np.random.default_rng(sum(shape) + 1000 * len(shape))
    if len(shape) == 3:
        G, N, W = shape
        return rng, _rand(rng, G * N, W), _rand(rng, G, W), 1, N, (), G, W
    O, M, G, Sn, W = shape
    return rng, _rand(rng, O, M, G * Sn, W), _rand(rng, O, G, W), M, Sn, (O,), G, W


SCORE_SHAPES = SC.SCORE_SHAPES + [s for s in SC.SHAPES if s not in SC.SCORE_SHAPES] + [SC.ENSEMBLE]


@pytest.mark.parametrize('shape', SCORE_SHAPES, ids=str)
def test_sample_crps(shape):
    rng, ys, target, M, Sn, lead, G, W = _pooled_inputs(shape)
    g = _rand(rng, *lead, G, W)

    def both():
        engine.sample_crps(ys, Sn, target, True, M, rank=True)
        engine.sample_crps_backward(g, ys, target, Sn, True, M, grad_target=True)
    run(f'{shape}', both, 'snsde_sample_crps', 'snsde_sample_crps_backward')
    if shape == SCORE_SHAPES[1]:    # the optional outputs absent: rank, ties and grad_target NULL; the biased estimator
        def bare():
            engine.sample_crps(ys, Sn, target, False, M, rank=False)
            engine.sample_crps_backward(g, ys, target, Sn, False, M, grad_target=False)
        run(f'{shape} crps only', bare, 'snsde_sample_crps', 'snsde_sample_crps_backward')


@pytest.mark.parametrize('shape', SCORE_SHAPES, ids=str)
def test_sample_quantiles(shape):
    rng, ys, target, M, Sn, lead, G, W = _pooled_inputs(shape)
    ks, fracs = engine.quantile_positions(SC.QS, M * Sn)
    g = _rand(rng, len(ks), *lead, G, W)

    def both():
        engine.sample_quantiles(ys, Sn, SC.QS, M)
        engine.sample_quantiles_backward(g, ys, Sn, ks, fracs, M)
    run(f'{shape}', both, 'snsde_sample_quantiles', 'snsde_sample_quantiles_backward')


@pytest.mark.parametrize('path', [False, True], ids=['vector', 'path'])
@pytest.mark.parametrize('shape', SC.ENERGY_SHAPES + [SC.ENSEMBLE], ids=str)
def test_sample_energy(shape, path):
    rng, ys, target, M, Sn, lead, G, W = _pooled_inputs(shape)
    g = _rand(rng, *(() if path else lead), G)

    def both():
        engine.sample_energy(ys, Sn, target, True, M, path)
        engine.sample_energy_backward(g, ys, target, Sn, True, M, path, grad_target=True)
    run(f'{shape} path={path}', both, 'snsde_sample_energy', 'snsde_sample_energy_backward')
    if shape == SC.ENERGY_SHAPES[1]:
        run(f'{shape} path={path} no grad_target', lambda: engine.sample_energy_backward(g, ys, target, Sn, False, M, path, grad_target=False),
            'snsde_sample_energy_backward')


@pytest.mark.parametrize('norm', [False, True], ids=['sum', 'norm'])
@pytest.mark.parametrize('shape', SC.LOGLIK_SHAPES, ids=str)
def test_sample_loglik(shape, norm):
    G, N, O, W = shape
    rng = np.random.default_rng(G + 7 * N + 31 * O + 101 * W)
    target = _rand(rng, O, G, W)
    ys = target.reshape(O, G, 1, W).add(0.4 * _rand(rng, O, G, N, W)).reshape(O, G * N, W).contiguous()
    mask = _dev((rng.random((O, G, W)) > 0.4).astype(np.float32))
    if G >= 2:
        mask[:, 0], mask[:, 1] = 0.0, 1.0      # a fully masked group and a fully observed one
    lw, gl, gb = 0.5 * _rand(rng, G, N), _rand(rng, G, N), _rand(rng, G)

    def both():
        bound, logpx, count, sqerr = engine.sample_loglik(ys, N, target, mask, 0.3, 1, lw, norm, stats=True)
        engine.sample_loglik_backward(gl, gb, ys, target, mask, logpx, count, N, 0.3, 1, lw, norm, True, True)
    run(f'{shape} norm={norm}', both, 'snsde_sample_loglik', 'snsde_sample_loglik_backward')
    if shape == SC.LOGLIK_SHAPES[1] and not norm:      # no weights, one upstream gradient, no optional gradient
        def bare():
            bound, logpx, count, sqerr = engine.sample_loglik(ys, N, target, mask, 0.3, 1, None, norm, stats=True)
            engine.sample_loglik_backward(None, gb, ys, target, mask, logpx, count, N, 0.3, 1, None, norm, False, False)
        run(f'{shape} bare', bare, 'snsde_sample_loglik', 'snsde_sample_loglik_backward')


@pytest.mark.parametrize('shape', CR.SHAPES, ids=str)
def test_sample_class(shape):
    G, N, O, Cn = shape
    c = CR.make_case(shape)
    z, y, lw, cw = _dev(c['z']), _dev(c['y']), _dev(c['lw']), _dev(c['cw'])
    gn, gx, gl = _dev(c['gn']), _dev(c['gx']), _dev(c['gl'])

    def both():
        engine.sample_class(z, N, y, 1, c['binary'], cw, lw, stats=True)
        engine.sample_class_backward(gn, gx, gl, z, N, y, 1, c['binary'], cw, lw, True)
    run(f'{shape}', both, 'snsde_sample_class', 'snsde_sample_class_backward')
    if shape == CR.SHAPES[2]:       # pure prediction and the plain loss: labels, weights and two of the upstream gradients NULL
        def bare():
            engine.sample_class(z, N, None, 1, c['binary'], None, None, stats=True)
            engine.sample_class_backward(gn, None, None, z, N, y, 1, c['binary'], None, None, False)
        run(f'{shape} bare', bare, 'snsde_sample_class', 'snsde_sample_class_backward')


# ---- splines and the head ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', SG.KINDS)
@pytest.mark.parametrize('key', SG.CASE_KEYS, ids=str)
def test_spline_coefficients_and_evaluation(key, kind):
    c = SG.case(*key)
    times, X, g = _dev(c['times'].astype(np.float32)), _dev(c['X'].astype(np.float32)), _dev(c['g'].astype(np.float32))
    L = key[0]

    def all_():
        coeffs = engine._spline_coeffs(times, X, kind)
        engine.spline_coeffs_backward(times, X, g, kind)
        return coeffs
    name = 'snsde_natural_cubic_coeffs' if kind == 'natural' else 'snsde_hermite_coeffs'
    run(f'{key} {kind}', all_, name, name + '_backward')
    coeffs = engine._spline_coeffs(times, X, kind)
    for derivative in (False, True):
        run(f'{key} {kind} derivative={derivative}', lambda: engine.spline_evaluate(coeffs, (L - 2) // 2, 0.3, derivative),
            'snsde_spline_evaluate')


@pytest.mark.parametrize('kind', HEAD_KINDS)
@pytest.mark.parametrize('shape', HEAD_SHAPES, ids=str)
def test_readout_head(kind, shape):
    lead, H, Hh, O = shape
    head, layers = make_head(kind, shape, DEV)
    x = torch.randn(*lead, H, device=DEV) * 2
    with torch.no_grad():
        run(f'{kind} {shape}', lambda: engine.readout_head(x, layers), 'snsde_readout_head')


# ---- composed parameter blocks: a call writes its jobs' ranges and nothing else -------------------------------------------------------

def _job_ranges(jobs, backward):
    """The (first float, one past the last float) ranges of dst (forward) or grad_src (backward) the jobs write."""
    out = []
    for q in jobs:
        cout = q.Cin + (1 if q.zero_col >= 0 else 0)
        if not backward:
            out.append((q.dst_w, q.dst_w + q.R * cout))
            if q.dst_b >= 0:
                out.append((q.dst_b, q.dst_b + q.R))
        elif not q.w_outer:
            out += [(o, o + n) for o, n in ((q.g_w_inner, q.R * q.Cin), (q.g_b_inner, q.R)) if o >= 0]
        else:
            out += [(o, o + n) for o, n in ((q.g_w_outer, q.R * q.K), (q.g_b_outer, q.R), (q.g_w_inner, q.K * q.Cin), (q.g_b_inner, q.K))
                    if o >= 0]
    return out


def hold_affine(what, name, jobs, inputs, out_numel, grad_dst=None, engine_out=None):
    """Assertions 1, 2, 5 and 6 on snsde_affine_compose (grad_dst None) or its backward.  inputs: the tensors behind the jobs'
    pointers.  engine_out: {(first, last): tensor}, what the engine's own call left in those ranges (assertion 4), or None."""
    backward = grad_dst is not None
    out = torch.empty(out_numel, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    args = (jobs, len(jobs)) + ((grad_dst.data_ptr(),) if backward else ()) + (out.data_ptr(), stream)
    known = {t.data_ptr(): t for t in inputs + ([grad_dst] if backward else [])}
    call = RecordedCall(name, args, 0, known, set())
    extra, pointer_args = {out.data_ptr(): (out, True)}, ((2, 3) if backward else (2,))
    ranges = _job_ranges(jobs, backward)
    assert all(0 <= a < b <= out_numel for a, b in ranges)
    written = torch.zeros(out_numel, dtype=torch.bool, device=DEV)
    for a, b in ranges:
        written[a:b] = True
    assert not bool(written.all()), 'the case leaves nothing unwritten: the rule has nothing to show'
    fn = getattr(_lib.lib(), name)
    got = {}
    for offset in (0, 1):
        for fill in FILLS:
            tag = f'{what} {name} fill {fill:#04x} offset {offset}'
            arena = _arena(call, fill, extra=[out])
            placed = place(call, arena, offset, extra, pointer_args)
            rc = replay(fn, call, placed, pointer_args)
            _sync()
            assert rc == 0, (tag, rc)
            arena.check(tag)
            for p in placed.values():
                if not p.is_output:
                    assert same_bits(p.view, p.original.reshape(-1)), f'{tag}: an input was changed'
            res = placed[out.data_ptr()].view.clone()
            untouched = res.view(torch.uint8).reshape(-1, 4)[~written]
            assert bool((untouched == fill).all()), f'{tag}: a float no job writes was written'
            got[offset, fill] = res[written]
            COMBINATIONS['count'] += 1
        for fill in FILLS[1:]:
            assert same_bits(got[offset, fill], got[offset, 0]), f'{what} {name} offset {offset}: a written float depends on the fill {fill:#04x}'
    same = same_bits(got[1, 0], got[0, 0])
    ALIGNMENT_SEEN.setdefault(name, []).append(same)
    print(f'{what} {name}: unaligned bits == aligned bits: {same}')
    if engine_out is not None:
        full = torch.zeros(out_numel, device=DEV)
        full[written] = got[0, 0]
        for (a, b), t in engine_out.items():
            assert same_bits(full[a:b], t.reshape(-1)), f'{what} {name}: floats {a} .. {b} differ from the engine\'s'


@pytest.mark.parametrize('kind,H,layers', COMPOSITION_CASES)
def test_affine_compose_of_the_tutorial_fields(kind, H, layers):
    B, Cn, L = 7, 3, 9
    pr = make_problem(900 + H, 4, 17, 2, B, H, Cn, L, times=np.linspace(0.0, 2.0, L))
    torch.manual_seed(900 + H)
    field = TutorialField(kind, Cn, H, layers, 'lipswish').to(DEV)
    field.set_X(torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['times']).to(DEV))
    cf = S.fields.compose(field)
    assert cf is not None
    cot = torch.randn(cf.numel, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    with recorded_calls(fields) as rec:
        flat = cf.flat(torch.device(DEV), grad=True)
        assert type(flat.grad_fn).__name__.startswith('_ComposeAffine')
        (flat * cot).sum().backward()
    _sync()
    fwd, bwd = rec.named('snsde_affine_compose'), rec.named('snsde_affine_compose_backward')
    assert fwd.rc == 0 and bwd.rc == 0
    jobs = fwd.args[0]
    params = [p for p in field.parameters()]
    by_ptr = {p.data_ptr(): p for p in params}
    used = [by_ptr[v] for q in jobs for v in (q.w_outer, q.b_outer, q.w_inner, q.b_inner) if v]
    flat_ranges = {r: flat.detach()[r[0]:r[1]] for r in _job_ranges(jobs, False)}
    hold_affine(f'{kind} H={H}', 'snsde_affine_compose', jobs, used, cf.numel, engine_out=flat_ranges)
    # the engine's gradient of a source tensor is what the call left at that tensor's g_* offset
    grads = {}
    for q in jobs:
        for ptr, off in ((q.w_outer, q.g_w_outer), (q.b_outer, q.g_b_outer), (q.w_inner, q.g_w_inner), (q.b_inner, q.g_b_inner)):
            if ptr and off >= 0:
                grads[off, off + by_ptr[ptr].numel()] = by_ptr[ptr].grad
    n_src = max(b for a, b in _job_ranges(jobs, True)) + 5
    hold_affine(f'{kind} H={H}', 'snsde_affine_compose_backward', jobs, used, n_src, grad_dst=cot.contiguous(), engine_out=grads)


def _hand_made(specs, seed):
    """Jobs from (R, K, Cin, zero_col, wanted) - K = 0: a copy job - with 3 floats nobody writes between any two ranges.
    wanted: which of (g_w_outer, g_b_outer, g_w_inner, g_b_inner) the backward is asked for."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)
    jobs, inputs, at, gat = (_lib.AffineJob * len(specs))(), [], 2, 1
    for q, (R, K, Cin, zero_col, wanted) in zip(jobs, specs):
        rows = K if K else R
        wi, bi = rnd(rows, Cin), rnd(rows)
        q.w_inner, q.b_inner, q.R, q.K, q.Cin, q.zero_col = wi.data_ptr(), bi.data_ptr(), R, K, Cin, zero_col
        inputs += [wi, bi]
        sizes = [0, 0, rows * Cin, rows]
        if K:
            wo, bo = rnd(R, K), rnd(R)
            q.w_outer, q.b_outer = wo.data_ptr(), bo.data_ptr()
            inputs += [wo, bo]
            sizes[:2] = [R * K, R]
        cout = Cin + (1 if zero_col >= 0 else 0)
        q.dst_w, q.dst_b = at, at + R * cout + 3
        at = q.dst_b + R + 3
        offs = []
        for n, want in zip(sizes, wanted):
            offs.append(gat if (n and want) else -1)
            gat += (n + 3) if (n and want) else 0
        q.g_w_outer, q.g_b_outer, q.g_w_inner, q.g_b_inner = offs
    return jobs, inputs, at, gat


ALL = (True, True, True, True)
HAND_MADE = {
    'R = 1, K = 1': [(1, 1, 3, -1, ALL)],
    'a zero column first and last, 258 columns': [(3, 2, 257, 0, ALL), (2, 0, 257, 257, ALL)],
    'twelve jobs, a copy last': [(2 + i % 3, 1 + i % 4, 5 + i, (i % 3) - 1, ALL if i != 4 else (False, True, True, False)) for i in range(11)]
                                + [(4, 0, 6, 1, ALL)],
}


@pytest.mark.parametrize('name', HAND_MADE)
def test_affine_compose_of_hand_made_jobs(name):
    specs = HAND_MADE[name]
    assert name != 'twelve jobs, a copy last' or len(specs) == _lib.MAX_AFFINE_JOBS
    jobs, inputs, n_dst, n_src = _hand_made(specs, 11)
    assert any(o == -1 for q in jobs for o in (q.g_w_outer, q.g_b_outer, q.g_w_inner, q.g_b_inner)) or len(specs) == 1
    hold_affine(name, 'snsde_affine_compose', jobs, inputs, n_dst)
    cot = torch.randn(n_dst, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    hold_affine(name, 'snsde_affine_compose_backward', jobs, inputs, n_src, grad_dst=cot)


def test_zz_report():
    """Prints what the tests above ran (after them, in file order): the number of combinations and, per function, whether the
    unaligned call gave the bits of the aligned one."""
    print(f'buffer contract: {COMBINATIONS["count"]} (function, shape, fill, alignment) combinations')
    for name, seen in sorted(ALIGNMENT_SEEN.items()):
        print(f'buffer contract: {name}: unaligned == aligned in {sum(seen)} of {len(seen)} calls'
              + (' (promised by include/snsde.h)' if name in ALIGNMENT_PROMISED else ''))
