"""Classification with sample paths on the host: the entry points snsde_sample_class / _backward (declared, exported, bound,
validating before they launch), and sample_class / mc_class_loss / evaluate_metrics on CPU tensors - the tensor-op statement of
the definition - against torch's own losses at S = 1, against the float64 numpy statement of tests/sample_class_reference.py,
the special values, and gradcheck.  No GPU compute.

Bounds: the statement runs in float64 here, so every comparison uses the bounds of tests/sample_class_reference.py with
u = 2^-53 and the depths of torch's sums (ops=True): float64 round-off alone."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine, train
from tests import sample_class_reference as R

ERR_NULL, ERR_DIMS = -1, -2
NAMES = ('snsde_sample_class', 'snsde_sample_class_backward')
KEYS = ('nll', 'xent', 'logp', 'probs', 'entropy', 'expected_entropy', 'mutual_information')
INF, NAN = float('inf'), float('nan')


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'snsde.h')).read()
    lib = _lib.lib()
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, arity in zip(NAMES, (17, 16)):
        assert f'SNSDE_API int {name}(' in header
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert f' T {name}\n' in dyn
        assert len(getattr(lib, name).argtypes) == arity
    assert lib.snsde_version() == 2      # (entry points added, no struct changed)
    assert S.sample_class is engine.sample_class and S.mc_class_loss is train.mc_class_loss


def _fwd(lib, outer=1, members=1, groups=1, samples=4, width=3, binary=0, logits=4096, logp=4096, nll=4096, xent=4096, probs=4096,
         entropy=4096, expent=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_class(p(logits), None, None, None, outer, members, groups, samples, width, binary, p(logp), p(nll), p(xent),
                                  p(probs), p(entropy), p(expent), None)


def _bwd(lib, outer=1, members=1, groups=1, samples=4, width=3, binary=0, logits=4096, grad_logits=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_class_backward(None, None, None, p(logits), None, None, None, outer, members, groups, samples, width, binary,
                                           p(grad_logits), None, None)


def test_the_entry_points_validate_before_they_launch():
    lib = _lib.lib()
    for name in ('logits', 'logp', 'nll', 'xent', 'probs', 'entropy', 'expent'):
        assert _fwd(lib, **{name: 0}) == ERR_NULL, name
    for name in ('logits', 'grad_logits'):
        assert _bwd(lib, **{name: 0}) == ERR_NULL, name
    for fn in (_fwd, _bwd):
        assert fn(lib, outer=0) == ERR_DIMS and fn(lib, members=0) == ERR_DIMS
        assert fn(lib, groups=0) == ERR_DIMS and fn(lib, samples=0) == ERR_DIMS
        assert fn(lib, width=0) == ERR_DIMS and fn(lib, groups=-3) == ERR_DIMS
        assert fn(lib, samples=257) == ERR_DIMS                                # N > 256
        assert fn(lib, samples=129, members=2) == ERR_DIMS                     # N = 258
        assert fn(lib, binary=1, width=2) == ERR_DIMS                          # binary stores one logit per path
        assert fn(lib, groups=2 ** 62, width=8) == ERR_DIMS                    # 63-bit overflow
        assert fn(lib, outer=2 ** 40, groups=2 ** 20, width=64) == ERR_DIMS
        assert fn(lib, logits=0, samples=257) == ERR_NULL                      # (pointers first, as the siblings)


def _worst(out, ref, keys=KEYS):
    return {k: R.worst(getattr(out, k).detach().numpy().reshape(ref[k].shape), ref[k], ref['E_' + k]) for k in keys}


# ---- known answers at S = 1 -----------------------------------------------------------------------------------------------------------------

def test_one_path_is_cross_entropy_and_bce_with_logits():
    gen = torch.Generator().manual_seed(1)
    B, Cn = 7, 5
    z = 3.0 * torch.randn(B, Cn, generator=gen, dtype=torch.float64)
    y = torch.randint(0, Cn, (B,), generator=gen)
    out = engine.sample_class_tensor_ops(z, 1, y, stats=True)
    want = F.cross_entropy(z, y, reduction='none')
    tol = 64 * R.U64 * (1.0 + want.abs().max())      # (log_softmax on both sides: a few roundings of values of this size)
    assert float((out.nll - want).abs().max()) <= tol and float((out.xent - want).abs().max()) <= tol
    assert float((out.logp[:, 0] + want).abs().max()) <= tol and float(out.mutual_information.abs().max()) <= tol
    cw = 0.5 + torch.rand(Cn, generator=gen, dtype=torch.float64)
    wout = engine.sample_class_tensor_ops(z, 1, y, class_weight=cw)
    assert float((wout - cw[y] * want).abs().max()) <= 2 * tol
    zb = 3.0 * torch.randn(B, 1, generator=gen, dtype=torch.float64)
    yb = torch.tensor([0, 1, 1, 0, 1, 0, 0])
    for pw in (1.0, 2.5):
        cwb = torch.tensor([1.0, pw], dtype=torch.float64)
        got = engine.sample_class_tensor_ops(zb, 1, yb, binary=True, class_weight=cwb, stats=True)
        wantb = F.binary_cross_entropy_with_logits(zb[:, 0], yb.double(), pos_weight=torch.tensor(pw, dtype=torch.float64), reduction='none')
        tolb = 64 * R.U64 * (1.0 + wantb.abs().max())
        assert float((got.nll - wantb).abs().max()) <= tolb and float((got.xent - wantb).abs().max()) <= tolb
        assert float((got.probs[:, 0] - torch.sigmoid(zb[:, 0])).abs().max()) <= tolb


# ---- the statement against the numpy reference -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(shape):
    return R.make_case(shape)


def _tensors(case, dtype=torch.float64):
    t = lambda k: torch.from_numpy(case[k]).to(dtype)
    return t('z'), torch.from_numpy(case['y']), t('lw'), t('cw')


@pytest.mark.parametrize('weights', [False, True])
@pytest.mark.parametrize('shape', R.SHAPES)
def test_the_statement_against_the_numpy_reference(shape, weights):
    G, N, O, Cn = shape
    case = _case(shape)
    z, y, lw, cw = _tensors(case)
    kw = dict(log_weight=lw, class_weight=cw) if weights else {}
    out = engine.sample_class_tensor_ops(z, N, y, binary=case['binary'], stats=True, **kw)
    ref = R.case_reference(shape, case, weights, u=R.U64, tiny=0.0, ops=True)
    assert tuple(out.nll.shape) == (O, G) and tuple(out.logp.shape) == (O, G, N)
    assert tuple(out.probs.shape) == (O, G, 1 if case['binary'] else Cn) and out.nll.dtype == torch.float64
    worst = _worst(out, ref)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert torch.equal(engine.sample_class(z, N, y, binary=case['binary'], **kw), out.nll)      # (CPU float64: the statement)
    assert float(out.mutual_information.min()) >= 0
    total = out.probs.sum(-1) if not case['binary'] else torch.ones(O, G, dtype=torch.float64)
    assert float((total - 1).abs().max()) <= float(ref['E_probs'].sum(-1).max())
    if not weights:      # (Jensen: the expected cross-entropy bounds the predictive NLL from above)
        assert bool((out.xent - out.nll >= -torch.from_numpy(ref['E_nll'] + ref['E_xent']).reshape(O, G)).all())
    if G >= 2:
        assert float(out.nll[:, 0].abs().max()) == 0 and float(out.xent[:, 0].abs().max()) == 0 and float(out.logp[:, 0].abs().max()) == 0


def test_identical_paths_have_no_epistemic_part():
    gen = torch.Generator().manual_seed(2)
    B, Sn, Cn = 4, 6, 5
    one = 3.0 * torch.randn(B, 1, Cn, generator=gen, dtype=torch.float64)
    z = one.expand(B, Sn, Cn).reshape(B * Sn, Cn).contiguous()
    y = torch.randint(0, Cn, (B,), generator=gen)
    out = engine.sample_class_tensor_ops(z, Sn, y, stats=True)
    ref = R.reference(z.numpy().reshape(B, Sn, Cn), y.numpy(), u=R.U64, tiny=0.0, ops=True)
    assert float((out.nll - out.xent).abs().max()) <= float((ref['E_nll'] + ref['E_xent']).max())
    assert float(out.mutual_information.max()) <= float(ref['E_mutual_information'].max())
    assert float((out.nll - F.cross_entropy(one[:, 0], y, reduction='none')).abs().max()) <= float(ref['E_nll'].max()) + 64 * R.U64 * 10


@pytest.mark.parametrize('binary', [False, True])
def test_a_per_path_shift_of_1e4_changes_nothing(binary):
    gen = torch.Generator().manual_seed(3)
    B, Sn, Cn = 3, 5, 1 if binary else 4
    z = 3.0 * torch.randn(B * Sn, Cn, generator=gen, dtype=torch.float64)
    y = torch.randint(0, 2 if binary else Cn, (B,), generator=gen)
    shift = 1e4 * (1.0 + torch.rand(B * Sn, 1, generator=gen, dtype=torch.float64))
    big = z + shift
    if binary:      # (the two logits of a path are (0, z): shifted together they are (c, z + c), i.e. a two-class row)
        z, big, binary = torch.cat([torch.zeros_like(z), z], 1), torch.cat([shift, z + shift], 1), False
    a = engine.sample_class_tensor_ops(z, Sn, y, stats=True)
    b = engine.sample_class_tensor_ops(big, Sn, y, stats=True)
    ref = R.reference(big.numpy().reshape(B, Sn, -1), y.numpy(), u=R.U64, tiny=0.0, ops=True)
    for k in KEYS:
        u, v = getattr(a, k), getattr(b, k)
        assert bool(torch.isfinite(v).all()), k
        # the shifted inputs are the sum z + 1e4 rounded: each logit moved by up to 2^-53 x 2e4, which every output follows 1-Lipschitz
        # (twice for differences of two), beside the bound of the computation itself
        slack = 4 * R.U64 * 2e4 * (1.0 + float(u.abs().max())) * 8
        assert float((u - v).abs().max()) <= float(np.max(ref['E_' + k])) + slack, k


# ---- special values -----------------------------------------------------------------------------------------------------------------------

def _special_inputs():
    gen = torch.Generator().manual_seed(4)
    G, N, Cn = 4, 3, 5
    z = 2.0 * torch.randn(G * N, Cn, generator=gen, dtype=torch.float64)
    y = torch.tensor([1, 2, 0, 4])
    return G, N, Cn, z, y


def test_minus_infinity_logits_are_classes_of_probability_zero():
    G, N, Cn, z, y = _special_inputs()
    z[0, 3] = z[1, 3] = -INF                     # group 0, a class that is not the label
    z[N + 1, 2] = -INF                           # group 1, path 1: the label's class
    zr = z.clone().requires_grad_(True)
    out = engine.sample_class_tensor_ops(zr, N, y, stats=True)
    ref = R.reference(z.numpy().reshape(G, N, Cn), y.numpy(), grads=(np.ones(G), np.zeros(G), np.zeros((G, N))), u=R.U64, tiny=0.0, ops=True)
    assert all(v <= 1.0 for v in _worst(out, ref, ('nll', 'logp', 'probs', 'entropy', 'expected_entropy')).values())
    assert bool(torch.isfinite(out.nll).all()) and bool(torch.isfinite(out.entropy).all()) and bool(torch.isfinite(out.expected_entropy).all())
    assert float(out.logp[1, 1].detach()) == -INF and float(out.xent[1].detach()) == INF and bool(torch.isfinite(out.xent[[0, 2, 3]]).all())
    g, = torch.autograd.grad(out.nll.sum(), zr)
    assert bool(torch.isfinite(g).all())
    assert float(g[0, 3]) == 0 and float(g[1, 3]) == 0                          # zero probability, zero gradient
    assert float(g[N + 1].abs().max()) == 0 and float(g[N].abs().max()) > 0      # the path of weight zero; its neighbour carries the group
    assert R.worst(g.numpy().reshape(G, N, Cn), ref['grad_logits'], ref['E_grad_logits']) <= 1.0


@pytest.mark.parametrize('binary', [False, True])
def test_unlabelled_rows_are_exact_zeros_with_their_statistics_intact(binary):
    G, N, Cn, z, y = _special_inputs()
    if binary:
        z, y = z[:, :1].contiguous(), torch.tensor([1, 0, 0, 1])
    lw = 0.3 * torch.randn(G, N, dtype=torch.float64)
    full = engine.sample_class_tensor_ops(z, N, y, binary=binary, log_weight=lw, stats=True)
    part = y.clone()
    part[1] = -1
    part[3] = -7
    for labels in (part, part.to(torch.int8), None):
        zr, lr = z.clone().requires_grad_(True), lw.clone().requires_grad_(True)
        out = engine.sample_class_tensor_ops(zr, N, labels, binary=binary, log_weight=lr, stats=True)
        rows = [1, 3] if labels is not None else [0, 1, 2, 3]
        for t in (out.nll, out.xent, out.logp):
            assert float(t.detach()[rows].abs().max()) == 0
        for k in ('probs', 'entropy', 'expected_entropy', 'mutual_information'):
            assert torch.equal(getattr(out, k), getattr(full, k)), k
        gz, gl = torch.autograd.grad(out.nll.sum() + out.xent.sum() + out.logp.sum(), (zr, lr))
        for r in rows:
            assert float(gz[r * N:(r + 1) * N].abs().max()) == 0 and float(gl[r].abs().max()) == 0
        if labels is not None:
            assert torch.equal(out.nll[[0, 2]], full.nll[[0, 2]]) and float(gz[:N].abs().max()) > 0


def test_a_label_beyond_the_classes_gives_nan_in_its_group_only():
    G, N, Cn, z, y = _special_inputs()
    y[2] = Cn
    zr = z.clone().requires_grad_(True)
    out = engine.sample_class_tensor_ops(zr, N, y, stats=True)
    for t in (out.nll, out.xent, out.logp):
        assert bool(torch.isnan(t[2]).all()) and bool(torch.isfinite(t[[0, 1, 3]]).all())
    for k in ('probs', 'entropy', 'expected_entropy'):      # (they need no label)
        assert bool(torch.isfinite(getattr(out, k)).all()), k
    g, = torch.autograd.grad(out.nll[[0, 1, 3]].sum(), zr)
    assert bool(torch.isfinite(g).all())
    yb = torch.tensor([0, 1, 2, 1])
    outb = engine.sample_class_tensor_ops(z[:, :1].contiguous(), N, yb, binary=True, stats=True)
    assert bool(torch.isnan(outb.nll[2])) and bool(torch.isfinite(outb.nll[[0, 1, 3]]).all())


def test_a_nan_logit_poisons_its_own_group_only():
    G, N, Cn, z, y = _special_inputs()
    z[2 * N + 1, 4] = NAN
    out = engine.sample_class_tensor_ops(z, N, y, stats=True)
    ref = R.reference(z.numpy().reshape(G, N, Cn), y.numpy(), u=R.U64, tiny=0.0, ops=True)
    assert all(v <= 1.0 for v in _worst(out, ref).values())      # (NaN where the reference has NaN, and nowhere else)
    for k in ('nll', 'xent', 'entropy', 'expected_entropy', 'mutual_information'):
        t = getattr(out, k)
        assert bool(torch.isnan(t[2])) and bool(torch.isfinite(t[[0, 1, 3]]).all()), k
    assert bool(torch.isnan(out.probs[2]).all()) and bool(torch.isfinite(out.probs[[0, 1, 3]]).all())
    assert bool(torch.isnan(out.logp[2, 1])) and int(torch.isnan(out.logp).sum()) == 1


def test_pooled_members_equal_the_hand_pooled_tensor():
    O, M, G, Sn, Cn = 2, 3, 4, 2, 5
    gen = torch.Generator().manual_seed(5)
    z = 2.0 * torch.randn(O, M, G * Sn, Cn, generator=gen, dtype=torch.float64)
    y = torch.randint(0, Cn, (O, G), generator=gen)
    lw = 0.3 * torch.randn(O, G, M * Sn, generator=gen, dtype=torch.float64)
    flat = z.reshape(O, M, G, Sn, Cn).permute(0, 2, 1, 3, 4).reshape(O, G * M * Sn, Cn).contiguous()
    a = engine.sample_class_tensor_ops(z, Sn, y, members=M, log_weight=lw, stats=True)
    b = engine.sample_class_tensor_ops(flat, M * Sn, y, log_weight=lw, stats=True)
    for k in KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert tuple(a.logp.shape) == (O, G, M * Sn)


@pytest.mark.parametrize('binary', [False, True])
@pytest.mark.parametrize('objective', ['nll', 'xent'])
def test_gradcheck_of_the_statement(objective, binary):
    gen = torch.Generator().manual_seed(6)
    G, N, Cn = 3, 4, 1 if binary else 3
    z = torch.randn(G * N, Cn, generator=gen, dtype=torch.float64, requires_grad=True)
    lw = (0.3 * torch.randn(G, N, generator=gen, dtype=torch.float64)).requires_grad_(True)
    cw = torch.tensor([1.0, 2.5] if binary else [0.5, 1.0, 1.5], dtype=torch.float64)
    y = torch.tensor([1, -1, 0])
    fn = lambda a, b: getattr(engine.sample_class_tensor_ops(a, N, y, binary=binary, class_weight=cw, log_weight=b, stats=True), objective)
    assert torch.autograd.gradcheck(fn, (z, lw))
    out = engine.sample_class_tensor_ops(z, N, y, binary=binary, class_weight=cw, log_weight=lw, stats=True)
    assert not out.probs.requires_grad and not out.entropy.requires_grad and not out.mutual_information.requires_grad


def test_argument_errors_are_value_errors():
    z = torch.zeros(6, 3)
    y = torch.zeros(2, dtype=torch.int64)
    for bad in (lambda: S.sample_class(z, 4), lambda: S.sample_class(z, 3, torch.zeros(2)), lambda: S.sample_class(z, 3, y[:1]),
                lambda: S.sample_class(z, 3, y, binary=True), lambda: S.sample_class(z, 3, y, class_weight=torch.ones(2)),
                lambda: S.sample_class(z, 3, y, log_weight=torch.zeros(2, 2)), lambda: S.sample_class(z, 3, y, members=0),
                lambda: S.sample_class(z.long(), 3, y)):
        with pytest.raises(ValueError):
            bad()


# ---- train.mc_class_loss and the metrics ------------------------------------------------------------------------------------------------------

def test_mc_class_loss_shapes_errors_and_objectives():
    gen = torch.Generator().manual_seed(7)
    B, Sn, Cn, M = 5, 3, 4, 2
    z = torch.randn(B * Sn, Cn, generator=gen, dtype=torch.float64)
    y = torch.randint(0, Cn, (B,), generator=gen)
    st = engine.sample_class_tensor_ops(z, Sn, y, stats=True)
    assert torch.equal(S.mc_class_loss(Sn)(z, y), st.nll.mean())
    assert torch.equal(S.mc_class_loss(Sn, objective='expected')(z, y), st.xent.mean())
    # 'expected' is what replicating the labels gives
    rep = F.cross_entropy(z, y.repeat_interleave(Sn))
    assert float((S.mc_class_loss(Sn, objective='expected')(z, y) - rep).abs()) <= 64 * R.U64 * (1 + float(rep))
    cw = torch.tensor([0.5, 1.0, 1.5, 2.0], dtype=torch.float64)
    assert torch.equal(S.mc_class_loss(Sn, class_weight=cw)(z, y), engine.sample_class_tensor_ops(z, Sn, y, class_weight=cw).mean())
    zm = torch.randn(M, B * Sn, Cn, generator=gen, dtype=torch.float64)
    assert torch.equal(S.mc_class_loss(Sn, members=M)(zm, y), engine.sample_class_tensor_ops(zm, Sn, y, members=M).mean())
    # binary: (B S,) from SqueezeEnd, float 0 / 1 labels as the sepsis loader gives them; pos_weight as BCEWithLogitsLoss at S = 1
    zb = torch.randn(B * Sn, generator=gen, dtype=torch.float64)
    yb = torch.tensor([0.0, 1.0, 1.0, 0.0, 1.0], dtype=torch.float64)
    want = engine.sample_class_tensor_ops(zb[:, None], Sn, yb.long(), binary=True, class_weight=torch.tensor([1.0, 3.0], dtype=torch.float64))
    assert torch.equal(S.mc_class_loss(Sn, binary=True, pos_weight=3.0)(zb, yb), want.mean())
    assert torch.equal(S.mc_class_loss(Sn, binary=True, pos_weight=torch.tensor(3.0))(zb[:, None], yb), want.mean())
    one = S.mc_class_loss(1, binary=True, pos_weight=3.0)(zb[:B], yb)
    bce = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(3.0, dtype=torch.float64))(zb[:B], yb)
    assert float((one - bce).abs()) <= 64 * R.U64 * (1 + float(bce))
    loss = S.mc_class_loss(Sn)
    for pred, true in ((z[:-1], y), (z, y[:-1]), (z.reshape(B * Sn, 2, 2), y), (z, y[:, None]), (zm, y)):
        with pytest.raises(ValueError):
            loss(pred, true)
    with pytest.raises(ValueError):
        S.mc_class_loss(Sn, binary=True)(z, y)
    for kw in (dict(objective='elbo'), dict(pos_weight=2.0), dict(binary=True, pos_weight=2.0, class_weight=[1.0, 2.0]), dict(samples=0)):
        with pytest.raises(ValueError):
            S.mc_class_loss(**{'samples': Sn, **kw})
    zr = z.clone().requires_grad_(True)
    S.mc_class_loss(Sn)(zr, y).backward()
    assert bool(torch.isfinite(zr.grad).all()) and float(zr.grad.abs().max()) > 0


def _loader(logits, labels, batch):
    """Batches (coeffs, true_y, lengths) whose 'coefficients' are the logits themselves: the stub model returns them."""
    return [(logits[i:i + batch], labels[i:i + batch], torch.zeros(len(labels[i:i + batch]))) for i in range(0, len(labels), batch)]


def test_evaluate_metrics_reads_sample_paths():
    gen = torch.Generator().manual_seed(8)
    B, Sn, Cn = 10, 4, 3
    dev = torch.device('cpu')
    times = torch.zeros(2)
    # samples = 1: today's numbers, by hand
    z1 = torch.randn(B, Cn, generator=gen)
    y = torch.randint(0, Cn, (B,), generator=gen)
    model = lambda times, coeffs, lengths: coeffs[0]
    want_acc = float((z1.argmax(1) == y).double().mean())
    want_loss = float(sum(float(F.cross_entropy(z1[i:i + 4], y[i:i + 4])) * len(y[i:i + 4]) for i in range(0, B, 4)) / B)
    old = train.evaluate_metrics(_loader(z1, y, 4), model, times, F.cross_entropy, Cn, dev, {})
    new = train.evaluate_metrics(_loader(z1, y, 4), model, times, F.cross_entropy, Cn, dev, {}, samples=1, members=1)
    assert old.accuracy == new.accuracy == want_acc and old.loss == new.loss and abs(old.loss - want_loss) <= 1e-6
    assert np.array_equal(old.confusion, new.confusion) and 'predictive_nll' not in new and set(old) == set(new)
    # samples = S: the averaged probabilities
    zs = 2.0 * torch.randn(B, Sn, Cn, generator=gen)
    paths = lambda times, coeffs, lengths: coeffs[0].reshape(-1, Cn)
    pbar = torch.softmax(zs.double(), -1).mean(1)
    acc = float((pbar.argmax(1) == y).double().mean())
    nll = float(-torch.log(pbar[torch.arange(B), y]).mean())
    ent = -(pbar * pbar.log()).sum(-1)
    each = torch.softmax(zs.double(), -1)
    mi = float((ent + (each * each.log()).sum(-1).mean(1)).mean())
    got = train.evaluate_metrics(_loader(zs, y, 4), paths, times, S.mc_class_loss(Sn), Cn, dev, {}, samples=Sn)
    assert got.dataset_size == B and abs(got.accuracy - acc) < 1e-12
    assert abs(got.predictive_nll - nll) <= 1e-5 and abs(got.loss - nll) <= 1e-5 and abs(got.mutual_information - mi) <= 1e-5
    assert got.confusion.sum() == B and np.trace(got.confusion) == round(acc * B)
    with pytest.raises((ValueError, RuntimeError)):      # (what the call without the keyword does with these rows)
        train.evaluate_metrics(_loader(zs, y, 4), paths, times, S.mc_class_loss(Sn), Cn, dev, {})
    # two classes: pbar(1) > 0.5, and the ranking metrics of pbar(1)
    zb = 2.0 * torch.randn(B, Sn, generator=gen)
    yb = torch.tensor([0., 1., 1., 0., 1., 0., 0., 1., 1., 0.])
    squeezed = lambda times, coeffs, lengths: coeffs[0].reshape(-1)
    p1 = torch.sigmoid(zb.double()).mean(1)
    gotb = train.evaluate_metrics(_loader(zb, yb, 5), squeezed, times, S.mc_class_loss(Sn, binary=True), 2, dev, {}, samples=Sn)
    assert abs(gotb.accuracy - float(((p1 > 0.5).double() == yb.double()).double().mean())) < 1e-12
    auroc, ap = train.binary_ranking_metrics(p1.float(), yb)
    assert abs(gotb.auroc - auroc) <= 1e-6 and abs(gotb.average_precision - ap) <= 1e-6
    pos, neg = p1[yb == 1], p1[yb == 0]
    by_hand = float(((pos[:, None] > neg[None, :]).double() + 0.5 * (pos[:, None] == neg[None, :]).double()).mean())
    assert abs(gotb.auroc - by_hand) <= 1e-6
    want_nll = float(-torch.log(torch.where(yb == 1, p1, 1 - p1)).mean())
    assert abs(gotb.predictive_nll - want_nll) <= 1e-5 and np.isfinite(gotb.mutual_information)
