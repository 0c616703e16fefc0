"""snsde_sample_class and its adjoint on the GPU, through sample_class / mc_class_loss / evaluate_metrics.

Shapes (groups G, pooled paths N, outer, stored width C; C = 0: binary), tests/sample_class_reference.py: SHAPES.  The kernel's
buckets follow from (N, C) (plan() there restates them): L = min(64, least power of two >= C) lanes per row and R = 256 / L rows
at a time; GP groups per workgroup, 1 for C > 64, else the largest power of two <= max(1, R / N); RS = min(16, R / GP) row parts
of the column sums; TN = min(64, 256 / GP) lanes over the paths; the slab staged in LDS up to GP N C = 24576 floats.
(1, 1, 1, 1) | (1, 1, 1, 2) - the smallest cases (one class: lp = 0); (3, 5, 2, 3) - odd sizes and the outer stride (GP = 8, three
packs, the last partly empty); (2, 8, 1, 35) - the Speech Commands width (L = 64, 35 live lanes); (2, 8, 1, 64) | (2, 8, 1, 65) -
the last width of the one-column-per-lane layout and the first of the 256-column sweep; (1, 256, 1, 4) - the cap of N;
(2, 7, 1, 0) - binary (GP = 32, RS = 8 > N: empty parts); (9000, 2, 1, 2) - many groups, GP = 64; (5, 2, 1, 35) | (5, 3, 1, 35) -
GP 2 | 1 at R = 4, an odd number of groups in packs of two; (2, 4, 1, 32) | (2, 4, 1, 33) - L 32 | 64; (3, 8, 1, 10) |
(3, 9, 1, 10) - GP 2 | 1 and RS 8 | 16 at R = 16; (2, 128, 1, 2) - RS at its cap of 16 with R / GP = 128; (1, 64, 1, 4) |
(1, 65, 1, 4) - one | two paths in a lane of the TN = 64 path lanes; (1, 3, 1, 256) | (1, 3, 1, 257) - one | two columns per
thread of the 256-column sweep; (1, 96, 1, 256) | (1, 96, 1, 257) - the largest staged slab and the first that is read twice;
(3, 1, 1, 0) | (1, 256, 1, 0) - binary at GP = 256 | 1; (4100, 4, 1, 33) - more packs than the 4096-block grid (the stride);
(1, 9, 1, 4099) - a wide row: seventeen columns per lane in the online logsumexp, the slab not staged.
Where G >= 2, group 0 is unlabelled.  Each shape runs without and with logw / class_weight, and with the upstream gradient
arriving through nll, xent and logp alone and through all three.  The float64 references are computed once per (shape, weights,
gradient route) from the float32 inputs and shared.  The bounds are those tests/sample_class_reference.py derives from the
summation order in include/snsde.h (u = 2^-24); the routing test uses the float32 tensor-op statement's bounds (ops=True)."""
import copy
import functools

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine, train
from tests import sample_class_reference as R
from tests.helpers import make_problem

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
KEYS = ('nll', 'xent', 'logp', 'probs', 'entropy', 'expected_entropy', 'mutual_information')
INF, NAN = float('inf'), float('nan')


@functools.lru_cache(maxsize=None)
def _case(shape):
    return R.make_case(shape)


@functools.lru_cache(maxsize=None)
def _ref(shape, weights, which):
    return R.case_reference(shape, _case(shape), weights, which)


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _np(t):
    return t.detach().double().cpu().numpy()


def _worst(out, ref, keys=KEYS):
    return {k: R.worst(_np(getattr(out, k)).reshape(ref[k].shape), ref[k], ref['E_' + k]) for k in keys}


def _inputs(shape, weights):
    c = _case(shape)
    kw = dict(log_weight=_dev(c['lw']), class_weight=_dev(c['cw'])) if weights else {}
    return c, _dev(c['z']), _dev(c['y']), kw


@pytest.mark.parametrize('weights', [False, True])
@pytest.mark.parametrize('shape', R.SHAPES)
def test_forward_against_float64(shape, weights):
    G, N, O, Cn = shape
    c, z, y, kw = _inputs(shape, weights)
    out = S.sample_class(z, N, y, binary=c['binary'], stats=True, **kw)
    ref = _ref(shape, weights, 'all')
    assert tuple(out.nll.shape) == tuple(out.entropy.shape) == (O, G) and tuple(out.logp.shape) == (O, G, N)
    assert tuple(out.probs.shape) == (O, G, 1 if c['binary'] else Cn) and all(t.dtype == torch.float32 for t in out)
    assert all(bool(torch.isfinite(t).all()) for t in out)
    worst = _worst(out, ref)
    print(f'sample_class {shape} weights={weights}: err / bound max ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    for a, b in zip(S.sample_class(z, N, y, binary=c['binary'], stats=True, **kw), out):      # two launches, the same bits
        assert torch.equal(a, b)
    assert torch.equal(S.sample_class(z, N, y, binary=c['binary'], **kw), out.nll)
    assert float(out.mutual_information.min()) >= 0
    if G >= 2:
        assert float(out.nll[:, 0].abs().max()) == 0 and float(out.xent[:, 0].abs().max()) == 0 and float(out.logp[:, 0].abs().max()) == 0
    pure = S.sample_class(z, N, None, binary=c['binary'], stats=True, **kw)      # labels=None: prediction alone
    assert float(pure.nll.abs().max()) == 0 and float(pure.logp.abs().max()) == 0
    for k in ('probs', 'entropy', 'expected_entropy'):
        assert torch.equal(getattr(pure, k), getattr(out, k)), k


@pytest.mark.parametrize('weights', [False, True])
@pytest.mark.parametrize('shape', R.SHAPES)
def test_gradients_against_the_float64_formulas(shape, weights):
    G, N, O, Cn = shape
    c, z0, y, kw0 = _inputs(shape, weights)
    gn, gx, gl = _dev(c['gn']), _dev(c['gx']), _dev(c['gl'])
    for which in ('nll', 'xent', 'logp', 'all'):
        z = z0.clone().requires_grad_(True)
        kw = dict(kw0)
        if weights:
            kw['log_weight'] = kw0['log_weight'].clone().requires_grad_(True)
        out = S.sample_class(z, N, y, binary=c['binary'], stats=True, **kw)
        assert type(out.nll.grad_fn).__name__.startswith('_SampleClass')
        assert not out.probs.requires_grad and not out.entropy.requires_grad and not out.mutual_information.requires_grad
        outs, gs = {'nll': ((out.nll,), (gn,)), 'xent': ((out.xent,), (gx,)), 'logp': ((out.logp,), (gl,)),
                    'all': ((out.nll, out.xent, out.logp), (gn, gx, gl))}[which]
        wrt = (z, kw['log_weight']) if weights else (z,)
        got = torch.autograd.grad(outs, wrt, gs)
        ref = _ref(shape, weights, which)
        worst = dict(grad_logits=R.worst(_np(got[0]).reshape(ref['grad_logits'].shape), ref['grad_logits'], ref['E_grad_logits']))
        if weights:
            worst['grad_logw'] = R.worst(_np(got[1]).reshape(ref['grad_logw'].shape), ref['grad_logw'], ref['E_grad_logw'])
        print(f'sample_class backward {shape} weights={weights} through {which}: err / bound max ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
        assert all(bool(torch.isfinite(t).all()) for t in got)
        assert all(v <= 1.0 for v in worst.values()), (which, worst)
        if G >= 2:      # the unlabelled group: exact zeros over its whole slab
            assert float(got[0].reshape(O, G, -1)[:, 0].abs().max()) == 0
            assert not weights or float(got[1][:, 0].abs().max()) == 0
        if which == 'all':      # engine.sample_class_backward: the same launch without autograd, and again: the same bits
            for _ in range(2):
                hz, hw = engine.sample_class_backward(gn, gx, gl, z.detach(), N, y, binary=c['binary'],
                                                      **{k: v.detach() for k, v in kw.items()})
                assert torch.equal(hz, got[0]) and (not weights or torch.equal(hw, got[1]))


# ---- special values ---------------------------------------------------------------------------------------------------------------------

def _special_inputs():
    gen = torch.Generator().manual_seed(4)
    G, N, Cn = 4, 3, 5
    z = 2.0 * torch.randn(G * N, Cn, generator=gen)
    y = torch.tensor([1, 2, 0, 4])
    return G, N, Cn, z, y


def _special_ref(z, y, N, grads=None, **kw):
    G = y.numel()
    return R.reference(z.double().numpy().reshape(G, N, -1), y.numpy(), grads=grads, **kw)


def test_minus_infinity_logits_are_classes_of_probability_zero():
    G, N, Cn, z, y = _special_inputs()
    z[0, 3] = z[1, 3] = -INF                     # group 0, a class that is not the label
    z[N + 1, 2] = -INF                           # group 1, path 1: the label's class
    zr = z.to(DEV).requires_grad_(True)
    out = S.sample_class(zr, N, y.to(DEV), stats=True)
    ref = _special_ref(z, y, N, grads=(np.ones(G), np.zeros(G), np.zeros((G, N))))
    worst = _worst(out, ref)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert bool(torch.isfinite(out.nll).all()) and bool(torch.isfinite(out.entropy).all()) and bool(torch.isfinite(out.expected_entropy).all())
    assert float(out.logp[1, 1].detach()) == -INF and float(out.xent[1].detach()) == INF
    g, = torch.autograd.grad(out.nll.sum(), zr)
    assert bool(torch.isfinite(g).all())
    assert float(g[0, 3]) == 0 and float(g[1, 3]) == 0                          # zero probability, zero gradient
    assert float(g[N + 1].abs().max()) == 0 and float(g[N].abs().max()) > 0      # the path of weight zero; its neighbour carries the group
    assert R.worst(_np(g).reshape(G, N, Cn), ref['grad_logits'], ref['E_grad_logits']) <= 1.0


def test_logits_of_magnitude_1e4_neither_overflow_nor_lose_the_answer():
    gen = torch.Generator().manual_seed(3)
    B, Sn, Cn = 3, 5, 4
    z = 3.0 * torch.randn(B * Sn, Cn, generator=gen) + 1e4 * (1.0 + torch.rand(B * Sn, 1, generator=gen))
    y = torch.randint(0, Cn, (B,), generator=gen)
    ref = _special_ref(z, y, Sn, grads=(np.ones(B), np.ones(B), np.zeros((B, Sn))))      # (of the float32 inputs as they stand)
    zr = z.to(DEV).requires_grad_(True)
    out = S.sample_class(zr, Sn, y.to(DEV), stats=True)
    assert all(bool(torch.isfinite(t).all()) for t in out)
    worst = _worst(out, ref)
    assert all(v <= 1.0 for v in worst.values()), worst
    g, = torch.autograd.grad(out.nll.sum() + out.xent.sum(), zr)
    assert R.worst(_np(g).reshape(B, Sn, Cn), ref['grad_logits'], ref['E_grad_logits']) <= 1.0
    zb = (1e4 * torch.tensor([1.0, -1.0, 0.5, -0.25, 1.0, 1.0])).reshape(6, 1)
    yb = torch.tensor([1, 0, 1])
    outb = S.sample_class(zb.to(DEV), 2, yb.to(DEV), binary=True, stats=True)
    refb = _special_ref(zb, yb, 2, binary=True)
    assert all(v <= 1.0 for v in _worst(outb, refb, ('logp', 'probs', 'entropy', 'expected_entropy')).values())
    assert float(outb.nll[2]) == 0.0 and not bool(torch.isnan(outb.nll).any())


@pytest.mark.parametrize('binary', [False, True])
def test_unlabelled_rows_are_exact_zeros_with_their_statistics_intact(binary):
    G, N, Cn, z, y = _special_inputs()
    if binary:
        z, y = z[:, :1].contiguous(), torch.tensor([1, 0, 0, 1])
    lw = (0.3 * torch.randn(G, N, generator=torch.Generator().manual_seed(9))).to(DEV)
    full = S.sample_class(z.to(DEV), N, y.to(DEV), binary=binary, log_weight=lw, stats=True)
    part = y.clone()
    part[1] = -1
    part[3] = -7
    for labels in (part.to(DEV), part.to(torch.int8).to(DEV), part.to(torch.int32).to(DEV), None):
        zr, lr = z.to(DEV).requires_grad_(True), lw.clone().requires_grad_(True)
        out = S.sample_class(zr, N, labels, binary=binary, log_weight=lr, stats=True)
        rows = [1, 3] if labels is not None else [0, 1, 2, 3]
        for t in (out.nll, out.xent, out.logp):
            assert float(t.detach()[rows].abs().max()) == 0 and not bool(torch.signbit(t.detach()[rows]).any())
        for k in ('probs', 'entropy', 'expected_entropy', 'mutual_information'):
            assert torch.equal(getattr(out, k), getattr(full, k)), k
        gz, gw = torch.autograd.grad(out.nll.sum() + out.xent.sum() + out.logp.sum(), (zr, lr))
        for r in rows:
            assert float(gz[r * N:(r + 1) * N].abs().max()) == 0 and float(gw[r].abs().max()) == 0
            assert not bool(torch.signbit(gz[r * N:(r + 1) * N]).any())
        if labels is not None:
            assert torch.equal(out.nll[[0, 2]], full.nll[[0, 2]]) and float(gz[:N].abs().max()) > 0


def test_a_label_beyond_the_classes_gives_nan_in_its_group_only():
    G, N, Cn, z, y = _special_inputs()
    clean = S.sample_class(z.to(DEV), N, y.to(DEV), stats=True)
    for beyond in (Cn, 2 ** 31 - 1, 2 ** 40):      # (no label value reaches an address)
        y2 = y.clone()
        y2[2] = beyond
        zr = z.to(DEV).requires_grad_(True)
        out = S.sample_class(zr, N, y2.to(DEV), stats=True)
        for k in ('nll', 'xent', 'logp'):
            t = getattr(out, k).detach()
            assert bool(torch.isnan(t[2]).all()) and torch.equal(t[[0, 1, 3]], getattr(clean, k)[[0, 1, 3]]), k
        for k in ('probs', 'entropy', 'expected_entropy'):      # (they need no label)
            assert torch.equal(getattr(out, k), getattr(clean, k)), k
        g, = torch.autograd.grad(out.nll.sum() + out.logp.sum(), zr)
        assert bool(torch.isnan(g[2 * N:3 * N]).all()) and bool(torch.isfinite(g[:2 * N]).all()) and bool(torch.isfinite(g[3 * N:]).all())
    yb = torch.tensor([0, 1, 2, 1])
    outb = S.sample_class(z[:, :1].contiguous().to(DEV), N, yb.to(DEV), binary=True, stats=True)
    assert bool(torch.isnan(outb.nll[2])) and bool(torch.isfinite(outb.nll[[0, 1, 3]]).all())


def test_a_nan_logit_poisons_its_own_group_only():
    G, N, Cn, z, y = _special_inputs()
    clean = S.sample_class(z.to(DEV), N, y.to(DEV), stats=True)
    z[2 * N + 1, 4] = NAN
    zr = z.to(DEV).requires_grad_(True)
    out = S.sample_class(zr, N, y.to(DEV), stats=True)
    ref = _special_ref(z, y, N)
    worst = _worst(out, ref)      # (NaN where the reference has NaN, and nowhere else)
    assert all(v <= 1.0 for v in worst.values()), worst
    keep = [0, 1, 3]
    for k in KEYS:
        a, b = getattr(out, k).detach(), getattr(clean, k)
        assert torch.equal(a[keep], b[keep]), k      # the other groups: the bits of the call without the NaN
        assert bool(torch.isnan(a[2]).any()), k
    assert bool(torch.isnan(out.probs[2]).all()) and bool(torch.isnan(out.logp[2, 1])) and int(torch.isnan(out.logp).sum()) == 1
    g, = torch.autograd.grad(out.nll[keep].sum(), zr)
    assert bool(torch.isfinite(g[:2 * N]).all()) and bool(torch.isfinite(g[3 * N:]).all())


# ---- determinism ------------------------------------------------------------------------------------------------------------------------

def test_pooled_ensemble_layout_gives_the_bits_of_the_permuted_single_member_call():
    O, M, G, Sn, Cn = 2, 2, 5, 4, 35
    gen = torch.Generator().manual_seed(3)
    z = 2.0 * torch.randn(O, M, G * Sn, Cn, generator=gen)
    y = torch.randint(0, Cn, (O, G), generator=gen).to(DEV)
    lw, gl = torch.randn(O, G, M * Sn, generator=gen), torch.randn(O, G, M * Sn, generator=gen)
    gn, gx = torch.randn(O, G, generator=gen).to(DEV), torch.randn(O, G, generator=gen).to(DEV)
    flat = z.reshape(O, M, G, Sn, Cn).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, Cn).contiguous()
    za, zb, la, lb = (t.to(DEV).requires_grad_(True) for t in (z, flat, lw, lw))
    a = S.sample_class(za, Sn, y, members=M, log_weight=la, stats=True)
    b = S.sample_class(zb, M * Sn, y, log_weight=lb, stats=True)
    for k in KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert tuple(a.logp.shape) == (O, G, M * Sn) and bool(torch.isfinite(a.nll).all())
    ga = torch.autograd.grad((a.nll, a.xent, a.logp), (za, la), (gn, gx, gl.to(DEV)))
    gb = torch.autograd.grad((b.nll, b.xent, b.logp), (zb, lb), (gn, gx, gl.to(DEV)))
    assert torch.equal(ga[0].reshape(O, M, G, Sn, Cn).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, Cn), gb[0])
    assert torch.equal(ga[1], gb[1]) and float(ga[0].abs().max()) > 0


def test_unaligned_and_non_contiguous_inputs_give_the_bits_of_their_clones():
    G, N, Cn = 4, 6, 35
    buf = torch.randn(G * N * Cn + 1, device=DEV)
    y = torch.tensor([3, 0, 34, 7], device=DEV)
    zu = buf[1:].reshape(G * N, Cn).requires_grad_(True)      # 4 bytes off a 16-byte boundary
    zc = buf[1:].clone().reshape(G * N, Cn).requires_grad_(True)
    a, b = S.sample_class(zu, N, y, stats=True), S.sample_class(zc, N, y, stats=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(torch.autograd.grad(a.nll.sum(), zu)[0], torch.autograd.grad(b.nll.sum(), zc)[0])
    wide = torch.randn(G * N, 2 * Cn, device=DEV).requires_grad_(True)
    zs = wide[:, ::2]
    zk = zs.detach().clone().requires_grad_(True)
    c1, c2 = S.sample_class(zs, N, y), S.sample_class(zk, N, y)
    assert not zs.is_contiguous() and torch.equal(c1, c2)
    g1, g2 = torch.autograd.grad(c1.sum(), wide)[0], torch.autograd.grad(c2.sum(), zk)[0]
    assert torch.equal(g1[:, ::2], g2) and float(g1[:, 1::2].abs().max()) == 0


# ---- routing ----------------------------------------------------------------------------------------------------------------------------

def test_routing_between_the_kernel_and_the_tensor_op_statement(monkeypatch):
    calls = []
    launch = engine._sample_class_launch
    monkeypatch.setattr(engine, '_sample_class_launch', lambda *a: (calls.append(1), launch(*a))[1])
    shape = (3, 5, 2, 3)
    G, N, O, Cn = shape
    c, z, y, kw = _inputs(shape, True)
    out = S.sample_class(z, N, y, stats=True, **kw)
    assert len(calls) == 1
    zr = z.clone().requires_grad_(True)
    assert type(S.sample_class(zr, N, y, **kw).grad_fn).__name__.startswith('_SampleClass') and len(calls) == 2
    ops = engine.sample_class_tensor_ops(z, N, y, stats=True, **kw)
    assert len(calls) == 2
    ref, ref_ops = _ref(shape, True, 'all'), R.case_reference(shape, c, True, ops=True)
    for k in KEYS:      # the kernel and the float32 statement on the same device: each within its own bound of float64
        assert R.worst(_np(getattr(ops, k)).reshape(ref[k].shape), ref_ops[k], ref_ops['E_' + k]) <= 1.0, k
        assert R.worst(_np(getattr(out, k)).reshape(ref[k].shape), _np(getattr(ops, k)).reshape(ref[k].shape), ref['E_' + k] + ref_ops['E_' + k]) <= 1.0, k
    # float64 and the CPU: the statement
    o64 = S.sample_class(z.double().requires_grad_(True), N, y, stats=True, log_weight=kw['log_weight'].double(), class_weight=kw['class_weight'].double())
    assert o64.nll.dtype == torch.float64 and not type(o64.nll.grad_fn).__name__.startswith('_SampleClass')
    cpu = S.sample_class(z.cpu(), N, y.cpu(), stats=True, log_weight=kw['log_weight'].cpu(), class_weight=kw['class_weight'].cpu())
    assert not cpu.nll.is_cuda and len(calls) == 2
    assert R.worst(_np(o64.nll).reshape(-1), ref['nll'], ref['E_nll']) <= 1.0
    # N = 257: beyond the kernels' cap
    N2, G2 = 257, 2
    gen = torch.Generator().manual_seed(5)
    z2 = torch.randn(G2 * N2, 4, generator=gen)
    y2 = torch.tensor([3, 1])
    zd = z2.to(DEV).requires_grad_(True)
    big = S.sample_class(zd, N2, y2.to(DEV), stats=True)
    assert len(calls) == 2 and big.nll.grad_fn is not None and not type(big.nll.grad_fn).__name__.startswith('_SampleClass')
    rb = R.reference(z2.double().numpy().reshape(G2, N2, 4), y2.numpy(), ops=True)
    assert all(v <= 1.0 for v in _worst(big, rb).values())
    gz, = torch.autograd.grad(big.nll.sum(), zd)
    assert bool(torch.isfinite(gz).all()) and float(gz.abs().max()) > 0
    S.sample_class(z2[:G2 * 256].to(DEV), 256, y2.to(DEV))      # N = 256: the kernel
    assert len(calls) == 3


# ---- capture ----------------------------------------------------------------------------------------------------------------------------

def test_captured_forward_and_backward_replay_to_the_eager_bits():
    G, N, Cn = 6, 8, 35
    gen = torch.Generator().manual_seed(6)
    draw = lambda: (2.0 * torch.randn(G * N, Cn, generator=gen).to(DEV), torch.randint(-1, Cn, (G,), generator=gen).to(DEV),
                    (0.3 * torch.randn(G, N, generator=gen)).to(DEV))
    cw = (0.5 + torch.rand(Cn, generator=gen)).to(DEV)

    def step(z, y, lw):
        out = S.sample_class(z, N, y, log_weight=lw, class_weight=cw, stats=True)
        gz, gw = torch.autograd.grad(out.nll.mean() + 0.5 * out.xent.mean(), (z, lw))
        return out.nll, out.mutual_information, gz, gw
    z0, y0, l0 = draw()
    sz, sy, sl = z0.clone().requires_grad_(True), y0.clone(), l0.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sz, sy, sl)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(sz, sy, sl)
    for _ in range(2):
        z1, y1, l1 = draw()
        with torch.no_grad():
            sz.copy_(z1); sy.copy_(y1); sl.copy_(l1)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(z1.requires_grad_(True), y1, l1.requires_grad_(True))
        for a, b in zip(held, eager):
            assert torch.equal(a, b)
        assert bool(torch.isfinite(eager[2]).all()) and float(eager[2].abs().max()) > 0


# ---- end to end -------------------------------------------------------------------------------------------------------------------------

TIMES = np.array([0., 1., 2., 3., 4., 5.], np.float32)


def test_a_classifier_trains_on_sample_paths_through_a_graphed_step_and_is_evaluated_on_them():
    Sn, B, H, Cn, classes = 4, 4, 64, 3, 3
    pr = make_problem(31, 4, 17, 2, B, H, Cn, len(TIMES), times=TIMES)
    torch.manual_seed(700)
    model, _ = S.make_sde_model('neurallnsde', Cn, classes, H, H, 2, initial=True)
    model.linear[3].p = 0.0      # (the head's dropout: eager and recorded steps would draw different masks)
    model = model.to(DEV).train()
    model2 = copy.deepcopy(model)
    coeffs, times = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)
    true = torch.tensor([2, 0, 1, 2], device=DEV)
    lengths = torch.full((B,), len(TIMES) - 1, device=DEV)
    kwargs = {'method': 'euler', 'options': {'seed': 9, 'samples': Sn, 'sample_grad': True}}
    base = S.mc_class_loss(Sn)
    seen = []

    def loss_fn(pred, y):
        assert tuple(pred.shape) == (B * Sn, classes)
        loss = base(pred, y)
        seen.append(loss.detach())      # (under capture: a view of the recording's loss, refreshed by every replay)
        return loss

    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    for _ in range(2):
        loss_fn(model(times, (coeffs,), lengths, **kwargs), true).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    eager = [t.clone() for t in seen]
    del seen[:]
    opt2 = torch.optim.Adam(model2.parameters(), lr=1e-3, capturable=True)
    graphed = train.GraphedStep(model2, times, opt2, loss_fn, kwargs, torch.device(DEV), warmup=1)
    graphed((coeffs,), true, lengths)      # the warm-up step of this batch shape: eager
    graphed((coeffs,), true, lengths)      # recorded, then replayed
    torch.cuda.synchronize()
    assert graphed.disabled is None and graphed.replays == 1, graphed.disabled
    assert len(seen) == 2 and torch.equal(seen[0], eager[0]) and torch.equal(seen[1], eager[1])
    assert bool(torch.isfinite(eager[1])) and not torch.equal(eager[0], eager[1])
    for p, p2 in zip(model.parameters(), model2.parameters()):      # the same Adam steps: the same gradients
        assert torch.equal(p, p2) and bool(torch.isfinite(p).all())
    model.eval()
    metrics = train.evaluate_metrics([(coeffs, true, lengths)], model, times, base, classes, torch.device(DEV), kwargs, samples=Sn)
    assert metrics.dataset_size == B and 0.0 <= metrics.accuracy <= 1.0 and metrics.confusion.sum() == B
    assert np.isfinite(metrics.loss) and np.isfinite(metrics.predictive_nll) and np.isfinite(metrics.mutual_information)
    assert abs(metrics.loss - metrics.predictive_nll) <= 1e-6 * (1 + abs(metrics.loss)) and metrics.mutual_information >= 0
