"""sample_loglik under a tensor noise on the host: a std / log_std per channel or per entry, the tensor-op statement against hand
answers and a brute-force float64 loop (forward and the four gradients), the maximum-likelihood property, select-never-multiply
for the noise, the argument errors, the entry points snsde_sample_loglik_noise / _backward / _reduce (declared, exported, bound,
validating before a launch), the scalar call left as it was, and the training layer (ObservationNoise, iwae_loss(noise=), one
train_loop epoch).  No GPU compute."""
import ctypes as C
import math
import os
import subprocess

import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine, train

ERR_NULL, ERR_DIMS = -1, -2
NAMES = ('snsde_sample_loglik_noise', 'snsde_sample_loglik_noise_backward', 'snsde_sample_loglik_noise_reduce')
LOG_2PI = math.log(2.0 * math.pi)


# ---- hand answers ------------------------------------------------------------------------------------------------------------------------

def test_hand_answers():
    """N = 1, W = 2, y = (1, 3), x = (0, 1): residuals (1, 2).  std = (1, 2): logpx = -1/2 (2 log 2 pi + 2 log 2 + 1 + 4 / 4) =
    -(log 2 pi + 1 + log 2) and d logpx / d ls = (1 - 1, 4 / 4 - 1) = (0, 0); std = (1, 1): the gradient is (0, 3)."""
    x = torch.tensor([[0.0, 1.0]], dtype=torch.float64)
    y = torch.tensor([[1.0, 3.0]], dtype=torch.float64)
    for std, grad in (((1.0, 2.0), (0.0, 0.0)), ((1.0, 1.0), (0.0, 3.0))):
        ls = torch.tensor(std, dtype=torch.float64).log().requires_grad_(True)
        bound, logpx, count, sqerr = S.sample_loglik(x, 1, y, log_std=ls, stats=True)
        if std == (1.0, 2.0):
            assert float(logpx.detach()) == pytest.approx(-(LOG_2PI + 1.0 + math.log(2.0)), rel=1e-15)
        assert torch.equal(bound, logpx[:, 0]) and float(count) == 2.0 and float(sqerr) == 5.0
        g, = torch.autograd.grad(logpx.sum(), ls)
        assert g.tolist() == pytest.approx(list(grad), abs=1e-15)
    # a tensor std is log_std = std.log(): the same value, and autograd chains through the logarithm (d / d std = (d / d ls) / std)
    st = torch.tensor([1.0, 1.0], dtype=torch.float64, requires_grad=True)
    a = S.sample_loglik(x, 1, y, std=st)
    assert torch.equal(a, S.sample_loglik(x, 1, y, log_std=torch.zeros(2, dtype=torch.float64)))
    assert torch.autograd.grad(a.sum(), st)[0].tolist() == pytest.approx([0.0, 3.0], abs=1e-15)
    # a 0-dim tensor is the (W,) vector of that value; the value of the scalar call
    b = S.sample_loglik(x, 1, y, log_std=torch.tensor(math.log(0.5), dtype=torch.float64))
    assert float(b) == pytest.approx(float(S.sample_loglik(x, 1, y, std=0.5)), rel=1e-14)


def test_the_gradient_vanishes_at_the_masked_mean_square_residual():
    """N = 1, no weights: d sum_b logpx / d ls_w = sum_b m_bw (d_bw^2 exp(-2 ls_w) - 1) = 0 exactly where exp(2 ls_w) is the masked
    mean square residual of channel w - the maximum-likelihood noise."""
    gen = torch.Generator().manual_seed(41)
    G, W = 7, 3
    x = torch.randn(G, W, generator=gen, dtype=torch.float64)
    y = torch.randn(G, W, generator=gen, dtype=torch.float64)
    m = (torch.rand(G, W, generator=gen) > 0.3).double()
    m[0] = 1.0
    msr = (m * (y - x) ** 2).sum(0) / m.sum(0)
    ls = (0.5 * msr.log()).requires_grad_(True)
    g, = torch.autograd.grad(S.sample_loglik(x, 1, y, m, log_std=ls).sum(), ls)
    assert float(g.abs().max()) <= 1e-13 * float(m.sum(0).max())
    off = (ls.detach() + 0.1).requires_grad_(True)      # a larger noise than the residuals ask for: the likelihood wants it smaller
    g, = torch.autograd.grad(S.sample_loglik(x, 1, y, m, log_std=off).sum(), off)
    assert bool((g < 0).all())


# ---- against a brute-force float64 loop --------------------------------------------------------------------------------------------------

def _case(seed, O, G, Sn, W, M=1, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    lead = (O,) if O else ()
    x = torch.randn(*lead, *((M,) if M > 1 else ()), G * Sn, W, generator=gen, dtype=dtype)
    y = torch.randn(*lead, G, W, generator=gen, dtype=dtype)
    m = (torch.rand(y.shape, generator=gen) > 0.4).to(dtype)
    lw = 0.5 * torch.randn(G, M * Sn, generator=gen, dtype=dtype)
    ls_c = 0.5 * torch.randn(W, generator=gen, dtype=dtype) - 0.5
    ls_e = 0.5 * torch.randn(y.shape, generator=gen, dtype=dtype) - 0.5
    return x, y, m, lw, ls_c, ls_e


def _loop(x, y, m, lw, ls, Sn, M, norm):
    """The definition as loops over python floats: (bound, logpx, d / d x, d / d y, d / d lw, d / d ls) of sum(bound) + sum(cos-weighted
    logpx) by the written-out adjoint."""
    O = x.shape[0]
    W = x.shape[-1]
    G = y.shape[1]
    N = M * Sn
    xs = x.reshape(O, M, G, Sn, W)
    entry = ls.dim() > 1
    logpx = torch.zeros(G, N, dtype=torch.float64)
    cnt = torch.zeros(G, dtype=torch.float64)
    for g in range(G):
        cnt[g] = sum(float(m[o, g, w]) for o in range(O) for w in range(W) if m[o, g, w] != 0)
        for n in range(N):
            mm, s = divmod(n, Sn)
            acc = 0.0
            for o in range(O):
                for w in range(W):
                    if m[o, g, w] != 0:
                        l = float(ls[o, g, w] if entry else ls[w])
                        d = float(y[o, g, w] - xs[o, mm, g, s, w])
                        acc += float(m[o, g, w]) * -0.5 * (LOG_2PI + 2.0 * l + d * d * math.exp(-2.0 * l))
            logpx[g, n] = acc / float(cnt[g]) if norm and cnt[g] > 0 else acc
    a = logpx + lw
    bound = torch.logsumexp(a, dim=-1) - math.log(N)
    p = torch.softmax(a, dim=-1)
    gl = torch.cos(logpx)                      # d / d logpx of sum(logpx * cos(logpx).detach())
    c = (gl + p) / (cnt.clamp(min=1.0)[:, None] if norm else 1.0)
    gx, gy, gls = torch.zeros_like(xs), torch.zeros_like(y), torch.zeros_like(ls)
    for g in range(G):
        for n in range(N):
            mm, s = divmod(n, Sn)
            for o in range(O):
                for w in range(W):
                    if m[o, g, w] != 0:
                        l = float(ls[o, g, w] if entry else ls[w])
                        d = float(y[o, g, w] - xs[o, mm, g, s, w])
                        t = float(c[g, n]) * float(m[o, g, w])
                        gx[o, mm, g, s, w] = t * d * math.exp(-2.0 * l)
                        gy[o, g, w] -= t * d * math.exp(-2.0 * l)
                        if entry:
                            gls[o, g, w] += t * (d * d * math.exp(-2.0 * l) - 1.0)
                        else:
                            gls[w] += t * (d * d * math.exp(-2.0 * l) - 1.0)
    return bound, logpx, gx.reshape(x.shape), gy, p, gls


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('entry', [False, True])
@pytest.mark.parametrize('M', [1, 2])
def test_both_modes_against_a_float64_loop_forward_and_all_four_gradients(M, entry, norm):
    O, G, Sn, W = 2, 3, 3, 4
    x, y, m, lw, ls_c, ls_e = _case(42 + M, O, G, Sn, W, M=M)
    m[:, 1, :] = 0.0 if norm else m[:, 1, :]      # (a row with nothing observed, under norm)
    ls = ls_e if entry else ls_c
    xr, yr, lwr, lsr = (t.clone().requires_grad_(True) for t in (x, y, lw, ls))
    bound, logpx, count, sqerr = S.sample_loglik(xr, Sn, yr, m, members=M, log_weight=lwr, norm=norm, stats=True, log_std=lsr)
    got = torch.autograd.grad(bound.sum() + (logpx * logpx.detach().cos()).sum(), (xr, yr, lwr, lsr))
    wb, wl, wx, wy, wp, wls = _loop(x, y, m, lw, ls, Sn, M, norm)
    bound, logpx = bound.detach(), logpx.detach()
    tol = lambda ref: 1e-12 * max(1.0, float(ref.abs().max()))
    assert float((logpx - wl).abs().max()) <= tol(wl) and float((bound - wb).abs().max()) <= tol(wb)
    for name, a, b in (('ys', got[0], wx), ('target', got[1], wy), ('log_weight', got[2], wp), ('log_std', got[3], wls)):
        assert a.shape == b.shape, name
        assert float((a - b).abs().max()) <= tol(b), name
    assert float(got[3].abs().max()) > 0
    # the tensor-op statement is what the call ran, and a tensor std is the same noise
    again = engine.sample_loglik_tensor_ops(x, Sn, y, m, members=M, log_weight=lw, norm=norm, stats=True, std=ls.exp())
    assert float((again[1] - logpx).abs().max()) <= tol(wl) and torch.equal(again[2], count)


# ---- select, never multiply --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('norm', [False, True])
def test_noise_at_unobserved_entries_reaches_nothing_and_receives_an_exact_zero(norm):
    O, G, Sn, W = 2, 3, 4, 5
    x, y, m, lw, ls_c, ls_e = _case(44, O, G, Sn, W, dtype=torch.float32)
    poison = torch.tensor([float('nan'), float('inf'), -float('inf')])
    hidden = m == 0
    outs, grads = [], []
    for planted in (False, True):
        ls = ls_e.clone()
        ls[hidden] = poison[torch.arange(int(hidden.sum())) % 3] if planted else 0.0
        xx, yy, ll = (t.clone().requires_grad_(True) for t in (x, y, ls))
        out = S.sample_loglik(xx, Sn, yy, m, log_std=ll, log_weight=lw, norm=norm, stats=True)
        outs.append(out)
        grads.append(torch.autograd.grad(out[0].sum() + (out[1] * out[1].detach().cos()).sum(), (xx, yy, ll)))
    for a, b in zip(outs[0], outs[1]):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    for a, b in zip(grads[0], grads[1]):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    gls = grads[1][2]
    assert float(gls[hidden].abs().max()) == 0 and not bool(torch.signbit(gls[hidden]).any())      # exact +0
    assert float(gls[~hidden].abs().min()) > 0
    # a fully masked channel: a NaN in its per-channel log-std reaches nothing either
    mc = m.clone()
    mc[..., 2] = 0.0
    lc = ls_c.clone()
    lc[2] = float('nan')
    lc.requires_grad_(True)
    out = S.sample_loglik(x, Sn, y, mc, log_std=lc, norm=norm, stats=True)
    g, = torch.autograd.grad(out[0].sum(), lc)
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all()) and float(g[2]) == 0 and bool(torch.isfinite(g).all())


def test_a_nan_log_std_at_an_observed_entry_poisons_its_own_row_only():
    G, Sn, W = 3, 4, 5
    x, y, m, lw, ls_c, ls_e = _case(45, 0, G, Sn, W)
    m[:] = 1.0
    ls_e[1, 3] = float('nan')
    bound, logpx, count, sqerr = S.sample_loglik(x, Sn, y, m, log_std=ls_e, stats=True)
    assert bool(torch.isnan(logpx[1]).all()) and bool(torch.isnan(bound[1]))
    assert bool(torch.isfinite(logpx[[0, 2]]).all()) and bool(torch.isfinite(bound[[0, 2]]).all())
    assert bool(torch.isfinite(sqerr).all()) and float(count[1]) == W      # (neither is weighed by the noise)


# ---- validation --------------------------------------------------------------------------------------------------------------------------

def test_argument_errors_are_value_errors():
    x, y = torch.zeros(12, 3), torch.zeros(4, 3)
    good = torch.zeros(3)
    for bad in (torch.zeros(4), torch.zeros(3, 4), torch.zeros(1, 4, 3), torch.zeros(2)):
        with pytest.raises(ValueError, match=r'\(3,\).*\(4, 3\)'):      # names both accepted shapes
            S.sample_loglik(x, 3, y, log_std=bad)
        with pytest.raises(ValueError, match=r'\(3,\).*\(4, 3\)'):
            S.sample_loglik(x, 3, y, std=bad + 1.0)
    for std in (0.2, 1, torch.ones(3), True, None):
        with pytest.raises(ValueError, match='std'):
            S.sample_loglik(x, 3, y, std=std, log_std=good)
    for ls in (0.0, [0.0, 0.0, 0.0], torch.zeros(3, dtype=torch.int64)):
        with pytest.raises(ValueError, match='log_std'):
            S.sample_loglik(x, 3, y, log_std=ls)
    for std in (torch.tensor([1.0, 0.0, 1.0]), torch.tensor([1.0, -1.0, 1.0]), torch.tensor([1.0, float('nan'), 1.0]), torch.tensor(0.0),
                torch.ones(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match='std'):
            S.sample_loglik(x, 3, y, std=std)
    with pytest.raises(ValueError, match='mask'):      # the other arguments are checked as ever
        S.sample_loglik(x, 3, y, torch.ones(4, 2), log_std=good)
    with pytest.raises(ValueError, match='log_weight'):
        S.sample_loglik(x, 3, y, log_std=good, log_weight=torch.zeros(3, 4))
    with pytest.raises(ValueError, match=r'\(3,\).*\(4, 3\)'):
        engine.sample_loglik_tensor_ops(x, 3, y, log_std=torch.zeros(5))
    assert S.sample_loglik(x, 3, y, log_std=good).shape == (4,)
    assert S.sample_loglik(x, 3, y, std=torch.ones(4, 3)).shape == (4,)
    assert S.sample_loglik(torch.zeros(2, 12, 3), 3, torch.zeros(2, 4, 3), log_std=torch.zeros(2, 4, 3)).shape == (4,)


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'snsde.h')).read()
    lib = _lib.lib()
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, arity in zip(NAMES, (17, 21, 6)):
        assert f'SNSDE_API int {name}(' in header
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert f' T {name}\n' in dyn
        assert len(getattr(lib, name).argtypes) == arity
    assert f'#define SNSDE_LOGLIK_NOISE_REDUCE_ROWS {_lib.LOGLIK_NOISE_REDUCE_ROWS}\n' in header
    assert f'#define SNSDE_NOISE_CHANNEL {_lib.NOISE_CHANNEL}\n' in header and f'#define SNSDE_NOISE_ENTRY {_lib.NOISE_ENTRY}\n' in header
    assert lib.snsde_version() == 2      # (entry points added, no struct changed)
    assert S.ObservationNoise is train.ObservationNoise


def _fwd(lib, outer=1, members=1, groups=1, samples=4, width=1, mode=0, ys=4096, target=4096, mask=4096, lstd=4096, logpx=4096,
         count=4096, bound=4096, sqerr=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_loglik_noise(p(ys), p(target), p(mask), None, p(lstd), outer, members, groups, samples, width, mode, 0,
                                         p(logpx), p(count), p(bound), p(sqerr), None)


def _bwd(lib, outer=1, members=1, groups=1, samples=4, width=1, mode=1, ys=4096, target=4096, mask=4096, lstd=4096, logpx=4096,
         count=4096, gys=4096):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.snsde_sample_loglik_noise_backward(None, None, p(ys), p(target), p(mask), None, p(lstd), p(logpx), p(count), outer, members,
                                                  groups, samples, width, mode, 1, p(gys), None, None, None, None)


def test_the_entry_points_validate_before_they_launch():
    """(Bogus non-NULL addresses: a call that launched would not return an argument error.)"""
    lib = _lib.lib()
    for fn in (_fwd, _bwd):
        for name in ('ys', 'target', 'mask', 'lstd', 'logpx', 'count'):
            assert fn(lib, **{name: 0}) == ERR_NULL, name
        assert fn(lib, outer=0) == ERR_DIMS and fn(lib, members=0) == ERR_DIMS
        assert fn(lib, groups=0) == ERR_DIMS and fn(lib, samples=0) == ERR_DIMS
        assert fn(lib, width=0) == ERR_DIMS and fn(lib, groups=-3) == ERR_DIMS
        assert fn(lib, samples=257) == ERR_DIMS and fn(lib, samples=129, members=2) == ERR_DIMS      # N > 256
        assert fn(lib, groups=2 ** 62, width=8) == ERR_DIMS                                          # 63-bit overflow
        assert fn(lib, outer=2 ** 40, groups=2 ** 20, width=64) == ERR_DIMS
        assert fn(lib, mode=2) == ERR_DIMS and fn(lib, mode=-1) == ERR_DIMS
    assert _fwd(lib, bound=0) == ERR_NULL and _fwd(lib, sqerr=0) == ERR_NULL
    assert _bwd(lib, gys=0) == ERR_NULL
    p = C.c_void_p
    red = lib.snsde_sample_loglik_noise_reduce
    assert red(None, 4, 4, None, p(4096), None) == ERR_NULL and red(p(4096), 4, 4, None, None, None) == ERR_NULL
    assert red(p(4096), 65, 4, None, p(4096), None) == ERR_NULL      # more than one block of rows needs the partial plane
    assert red(p(4096), 0, 4, None, p(4096), None) == ERR_DIMS and red(p(4096), 4, 0, None, p(4096), None) == ERR_DIMS
    assert red(p(4096), -1, 4, None, p(4096), None) == ERR_DIMS and red(p(4096), 2 ** 62, 8, p(4096), p(4096), None) == ERR_DIMS


# ---- the scalar call is as it was --------------------------------------------------------------------------------------------------------

def test_a_float_std_gives_the_values_of_the_tensor_op_statement_before_the_noise_arguments():
    """Recorded from the statement as it stood before std could be a tensor (seed 46, float32, std 0.3, with weights): the scalar
    branch is the same arithmetic, bit for bit - and log_std=None is part of the new signature."""
    O, G, Sn, W = 2, 3, 4, 5
    x, y, m, lw, _, _ = _case(46, O, G, Sn, W, dtype=torch.float32)
    for norm, want in ((False, RECORDED[0]), (True, RECORDED[1])):
        bound, logpx, count, sqerr = S.sample_loglik(x, Sn, y, m, std=0.3, log_weight=lw, norm=norm, stats=True, log_std=None)
        got = torch.stack([bound[0], bound[2], logpx[1, 3], sqerr[1]])
        assert torch.equal(got, torch.tensor(want, dtype=torch.float32)), [v.hex() for v in got.tolist()]
        again = engine.sample_loglik_tensor_ops(x, Sn, y, m, 0.3, 1, lw, norm, True, None)
        assert all(torch.equal(a, b) for a, b in zip(again, (bound, logpx, count, sqerr)))


RECORDED = (
    [float.fromhex(h) for h in ('-0x1.6e5244p+5', '-0x1.8a8792p+5', '-0x1.1b77d4p+4', '0x1.45f5fp+1')],      # bound[0], bound[2], logpx[1, 3], sqerr[1]
    [float.fromhex(h) for h in ('-0x1.116a88p+3', '-0x1.a722aep+2', '-0x1.c58c86p+1', '0x1.45f5fp+1')],      # ... under norm
)


# ---- the training layer ------------------------------------------------------------------------------------------------------------------

class _Toy(torch.nn.Module):
    """(times, coeffs, lengths) -> (B S, T, out): a linear map of the first coefficient tensor plus fixed per-path offsets."""

    def __init__(self, Sn, T, out):
        super().__init__()
        self.lin = torch.nn.Linear(2, T * out)
        self.Sn, self.T, self.out = Sn, T, out

    def forward(self, times, coeffs, lengths, **kwargs):
        z = self.lin(coeffs[0]).reshape(-1, 1, self.T, self.out)
        off = 0.1 * torch.arange(self.Sn, dtype=z.dtype).reshape(1, self.Sn, 1, 1)
        return (z + off).reshape(-1, self.T, self.out)


def test_observation_noise_owns_the_parameter_and_prefixes_the_model():
    net = train.ObservationNoise(_Toy(2, 3, 4), 4, std=0.5)
    assert isinstance(net.log_std, torch.nn.Parameter) and net.log_std.shape == (4,) and net.log_std.dtype == torch.float32
    assert torch.equal(net.log_std.detach(), torch.full((4,), math.log(0.5), dtype=torch.float32))
    assert any(p is net.log_std for p in net.parameters())
    assert sorted(net.state_dict()) == ['log_std', 'model.lin.bias', 'model.lin.weight']
    assert net.std.tolist() == pytest.approx([0.5] * 4, rel=1e-6)
    c = torch.randn(5, 2)
    assert torch.equal(net(None, [c], None), net.model(None, [c], None))
    assert train.ObservationNoise(_Toy(2, 3, 4), 4, per_step=3).log_std.shape == (3, 4)
    for kw in ({'channels': 0}, {'channels': 4, 'std': 0.0}, {'channels': 4, 'per_step': True}, {'channels': 4, 'per_step': 0}):
        with pytest.raises(ValueError):
            train.ObservationNoise(_Toy(2, 3, 4), **kw)


def test_iwae_loss_with_noise_is_the_per_channel_call_on_the_flattened_vector_and_follows_the_parameter():
    B, Sn, T, out = 3, 4, 5, 2
    gen = torch.Generator().manual_seed(47)
    pred = torch.randn(B * Sn, T, out, generator=gen, requires_grad=True)
    true = torch.randn(B, T, out, generator=gen)
    true[0, 1, 0] = true[2, :, 1] = float('nan')
    net = train.ObservationNoise(torch.nn.Identity(), out, std=0.5)
    with torch.no_grad():
        net.log_std.copy_(torch.tensor([-0.3, 0.4]))
    loss_fn = S.iwae_loss(Sn, noise=net)
    loss = loss_fn(pred, true)
    entry = net.log_std.detach().expand(B, T, out).reshape(B, T * out)      # the same noise written out per entry
    want = -S.sample_loglik(pred.reshape(B * Sn, -1), Sn, true.reshape(B, -1), log_std=entry).mean()
    assert loss.shape == () and bool(torch.isfinite(loss)) and float(loss) == pytest.approx(float(want), rel=1e-6)
    gp, gn = torch.autograd.grad(loss, (pred, net.log_std))
    assert gn.shape == (out,) and float(gn.abs().min()) > 0 and float(gp[torch.isnan(true).repeat_interleave(Sn, 0)].abs().max()) == 0
    with torch.no_grad():      # read at every call, not captured by value
        net.log_std.add_(0.25)
    assert float(loss_fn(pred, true)) != float(loss)
    assert float(loss_fn(pred, true)) == pytest.approx(
        float(-S.sample_loglik(pred.reshape(B * Sn, -1), Sn, true.reshape(B, -1), log_std=entry + 0.25).mean()), rel=1e-6)
    # a per-step scale, and any object with a .log_std
    step = train.ObservationNoise(torch.nn.Identity(), out, per_step=T)
    assert float(S.iwae_loss(Sn, noise=step)(pred, true)) == pytest.approx(float(S.iwae_loss(Sn, std=0.1)(pred, true)), rel=1e-5)

    class Bag:
        log_std = torch.zeros(out)
    assert float(S.iwae_loss(Sn, noise=Bag())(pred, true)) == pytest.approx(float(S.iwae_loss(Sn, std=1.0)(pred, true)), rel=1e-5)
    with pytest.raises(ValueError, match='std'):
        S.iwae_loss(Sn, std=0.5, noise=net)
    with pytest.raises(ValueError, match='log_std'):
        S.iwae_loss(Sn, noise=object())
    with pytest.raises(ValueError, match='log_std'):
        S.iwae_loss(Sn, noise=train.ObservationNoise(torch.nn.Identity(), 3))(pred, true)
    assert torch.equal(S.iwae_loss(Sn, std=0.5, noise=None)(pred, true), S.iwae_loss(Sn, std=0.5)(pred, true))


def test_one_train_loop_epoch_moves_log_std():
    B, Sn, T, out = 8, 2, 3, 2
    gen = torch.Generator().manual_seed(48)
    coeffs, true = torch.randn(B, 2, generator=gen), torch.randn(B, T, out, generator=gen)
    true[1, 0, 1] = float('nan')
    data = [(coeffs[:4], true[:4], torch.zeros(4)), (coeffs[4:], true[4:], torch.zeros(4))]
    net = train.ObservationNoise(_Toy(Sn, T, out), out, std=0.1)
    before = net.log_std.detach().clone()
    opt = torch.optim.Adam(net.parameters(), lr=0.05)
    hist = train.train_loop(data, data, net, None, opt, S.iwae_loss(Sn, noise=net), 1, None, 'cpu', {}, 'none')
    assert len(hist) == 1 and math.isfinite(hist[0].train_metrics.loss)
    assert float((net.log_std.detach() - before).abs().min()) > 0
    assert bool((net.log_std.detach() > before).all())      # residuals of order 1 under std = 0.1: the likelihood asks for more noise
