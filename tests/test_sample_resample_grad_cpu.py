"""The adjoint of the resampling step without a GPU (include/snsde.h: snsde_sample_resample_backward): the entry point's
declaration and its argument checks, and `sample_resample_tensor_ops(differentiable=True)` against float64 autograd through a plain
restatement written here (logsumexp, index_select) with the ancestors held fixed, torch.autograd.gradcheck, and the special rows
with exact zeros and exact pass-throughs."""
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
from tests.test_sample_resample_cpu import R_bits, special_cases, special_state

ERR_NULL, ERR_DIMS = -1, -2
INF, NAN = float('inf'), float('nan')
NAME = 'snsde_sample_resample_backward'


def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'snsde.h')).read()
    lib = _lib.lib()
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f'SNSDE_API int {NAME}(' in header
    assert NAME in _lib.EXPORTS and hasattr(lib, NAME)
    assert f' T {NAME}\n' in dyn
    assert len(getattr(lib, NAME).argtypes) == 13
    assert lib.snsde_version() == 2      # (an entry point added, no struct changed)
    assert callable(engine.sample_resample_backward)


def _call(lib, groups=1, samples=4, width=3, gso=1 << 12, glw=1 << 13, glz=1 << 14, logw=1 << 15, loginc=1 << 16, ancestor=1 << 17,
          resampled=1 << 18, grad_state=1 << 30, grad_a=1 << 31):
    """Dummy non-null pointers: every case here must be refused before anything is launched."""
    p = lambda v: C.c_void_p(v) if v else None
    return getattr(lib, NAME)(p(gso), p(glw), p(glz), p(logw), p(loginc), p(ancestor), p(resampled), groups, samples, width,
                              p(grad_state), p(grad_a), None)


def test_the_entry_point_validates_before_it_launches():
    lib = _lib.lib()
    for name in ('logw', 'ancestor', 'resampled', 'grad_state', 'grad_a'):
        assert _call(lib, **{name: 0}) == ERR_NULL, name
    assert _call(lib, samples=0) == ERR_DIMS and _call(lib, samples=257) == ERR_DIMS and _call(lib, width=0) == ERR_DIMS
    assert _call(lib, groups=0) == ERR_DIMS and _call(lib, groups=-3) == ERR_DIMS and _call(lib, samples=-1) == ERR_DIMS
    assert _call(lib, groups=2 ** 61, width=8) == ERR_DIMS and _call(lib, groups=2 ** 62, samples=1, width=1) == ERR_DIMS      # 63 bits
    assert _call(lib, logw=0, samples=257) == ERR_NULL      # (pointers first, as the forward)
    # an output overlapping an input, from the same pointer to the last byte - and the first byte past it is not
    nbytes, gs, g = 1 * 4 * 3 * 4, 1 * 4 * 4, 4
    at = 1 << 20
    for off in (0, 4, nbytes - 4, -4, -(nbytes - 4)):
        assert _call(lib, gso=at, grad_state=at + off) == ERR_DIMS, off
    for name, size in (('glw', gs), ('logw', gs), ('loginc', gs), ('ancestor', gs), ('glz', g), ('resampled', g)):
        for off in (0, size - 4, -(gs - 4)):
            assert _call(lib, **{name: at, 'grad_a': at + off}) == ERR_DIMS, (name, off)
        assert _call(lib, **{name: at, 'grad_state': at + size - 4}) == ERR_DIMS, name
    assert _call(lib, grad_state=at, grad_a=at + nbytes - 4) == ERR_DIMS and _call(lib, grad_state=at + 4, grad_a=at) == ERR_DIMS


# ---- the statement against a plain restatement ----------------------------------------------------------------------------------------------

def restate(x, lw, inc, anc, res, Sn):
    """The three differentiable outputs from fixed ancestors: x (G, S, W), lw, inc (G, S) float64 with a graph; anc, res constants."""
    a = lw if inc is None else lw + inc
    logz = torch.logsumexp(a, dim=-1) - math.log(Sn)
    rows, ws = [], []
    for g in range(x.shape[0]):
        rows.append(x[g].index_select(0, anc[g].long()) if int(res[g]) else x[g])
        ws.append(logz[g].expand(Sn) if int(res[g]) else a[g])
    return torch.stack(rows), torch.stack(ws), logz


def _inputs(shape, scale, dtype=torch.float64):
    c = R.make_case(shape, scale)
    G, Sn, W = shape
    t = lambda k: torch.from_numpy(c[k]).to(dtype)
    return t('state').reshape(G * Sn, W), t('logw'), t('loginc'), t('u'), t('us')


@pytest.mark.parametrize('threshold', [0.0, 0.5, 1.0])
@pytest.mark.parametrize('stratified', [False, True], ids=['systematic', 'stratified'])
@pytest.mark.parametrize('shape', [(2, 5, 3), (3, 1, 4), (4, 32, 8)], ids=str)
def test_the_statement_against_the_restatement(shape, stratified, threshold):
    G, Sn, W = shape
    x, lw, inc, u, us = _inputs(shape, 4.0)
    uu = us if stratified else u
    plain = engine.sample_resample_tensor_ops(x, Sn, lw, inc, uu, threshold, stratified)
    rng = torch.Generator().manual_seed(5)
    cs, cw, cz = (torch.randn(s, generator=rng, dtype=torch.float64) for s in ((G * Sn, W), (G, Sn), (G,)))
    for with_inc in (True, False):
        leaves = [t.clone().requires_grad_(True) for t in ((x, lw, inc) if with_inc else (x, lw))]
        out = engine.sample_resample_tensor_ops(leaves[0], Sn, leaves[1], leaves[2] if with_inc else None, uu, threshold, stratified,
                                                differentiable=True)
        if with_inc:      # the forward values of the differentiable statement are those of the plain one, bit for bit
            for a, b in zip(out, plain):
                assert R_bits(a.detach(), b)
        assert not (out.ancestor.requires_grad or out.ess.requires_grad or out.resampled.requires_grad)
        got = torch.autograd.grad((out.state * cs).sum() + (out.log_weight * cw).sum() + (out.logz * cz).sum(), leaves)
        ref_leaves = [t.clone().requires_grad_(True) for t in ((x, lw, inc) if with_inc else (x, lw))]
        rs, rw, rz = restate(ref_leaves[0].reshape(G, Sn, W), ref_leaves[1], ref_leaves[2] if with_inc else None, out.ancestor, out.resampled, Sn)
        want = torch.autograd.grad((rs.reshape(G * Sn, W) * cs).sum() + (rw * cw).sum() + (rz * cz).sum(), ref_leaves)
        for a, b in zip(got, want):
            assert torch.allclose(a, b, rtol=1e-12, atol=1e-14), float((a - b).abs().max())
        if with_inc:
            assert torch.equal(got[1], got[2])      # one gradient for a = log_weight + log_increment


def test_gradcheck():
    shape = (2, 5, 3)
    G, Sn, W = shape
    x, lw, inc, u, us = _inputs(shape, 1.0)
    for stratified, uu in ((False, u), (True, us)):
        for threshold in (0.0, 1.0):
            def fn(xs, l, i):
                o = engine.sample_resample_tensor_ops(xs, Sn, l, i, uu, threshold, stratified, differentiable=True)
                return o.state, o.log_weight, o.logz
            # (the ancestors are piecewise constant in the weights: the finite differences of gradcheck stay inside one piece, which
            # the reference's margin states for this seed)
            ref = R.reference(lw.numpy(), inc.numpy(), uu.numpy(), threshold, stratified, unit=R.U64)
            assert threshold == 0.0 or float(ref['margin'].min()) > 1e-4
            leaves = [t.clone().requires_grad_(True) for t in (x, lw, inc)]
            assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-6)


def test_the_default_still_refuses_and_the_opt_in_does_not():
    x, lw, u = torch.zeros(8, 3), torch.zeros(2, 4), torch.full((2,), 0.5)
    for fn in (S.sample_resample, engine.sample_resample_tensor_ops):
        with pytest.raises(ValueError, match='inference only.*requires grad'):
            fn(x.clone().requires_grad_(True), 4, lw, u=u, differentiable=False)
        out = fn(x.clone().requires_grad_(True), 4, lw.clone().requires_grad_(True), u=u, threshold=1.0, differentiable=True)
        assert out.state.requires_grad and out.log_weight.requires_grad and out.logz.requires_grad
        assert not (out.ancestor.requires_grad or out.ess.requires_grad or out.resampled.requires_grad)
        with torch.no_grad():
            assert not fn(x.clone().requires_grad_(True), 4, lw, u=u, differentiable=True).state.requires_grad


# ---- special rows ---------------------------------------------------------------------------------------------------------------------------

def special_gradients(fn, name, dtype, device='cpu', nan_row=None):
    """The gradients of one special case through `fn` (sample_resample or its statement) under fixed output gradients.  Returns
    (out, grad_state (G, S, W), grad_logw, cs, cw, cz); nan_row puts a NaN into that row of the state's output gradient."""
    rows, u, _ = special_cases()[name]
    lw = torch.tensor(rows, dtype=dtype, device=device).requires_grad_(True)
    x = special_state().to(dtype).to(device).requires_grad_(True)
    ud = torch.tensor(u, dtype=dtype, device=device)
    rng = torch.Generator().manual_seed(11)
    cs, cw, cz = (torch.randn(s, generator=rng, dtype=torch.float64).to(dtype).to(device) for s in ((12, 3), (3, 4), (3,)))
    if nan_row is not None:
        cs[nan_row, 1] = NAN
    out = fn(x, 4, lw, None, ud, 1.0, differentiable=True)
    gx, gl = torch.autograd.grad([out.state, out.log_weight, out.logz], [x, lw], [cs, cw, cz])
    return out, gx.reshape(3, 4, 3), gl, cs.reshape(3, 4, 3), cw, cz


def check_special_gradients(name, out, gx, gl, cs, cw, cz):
    """Row 1 of a special case: exact zeros for a dead particle, exact pass-through for a row that was left as it is."""
    rows, _, kind = special_cases()[name]
    lw = torch.tensor(rows[1], dtype=gl.dtype)      # (dead in the dtype of the run: exp(-300) is 0 in float32 only)
    if kind == 'live':
        assert int(out.resampled[1]) == 1, name
        dead = (torch.exp(lw - lw.max()) == 0).tolist()
        assert any(dead) or gl.dtype == torch.float64, name
        for n, is_dead in enumerate(dead):
            if is_dead:
                assert torch.equal(gl[1, n].cpu(), torch.zeros((), dtype=gl.dtype)), (name, n, float(gl[1, n]))
                assert torch.equal(gx[1, n].cpu(), torch.zeros(3, dtype=gx.dtype)), (name, n)
        assert bool(torch.isfinite(gl[1]).all()) and bool(torch.isfinite(gx[1]).all()), name
    else:
        assert int(out.resampled[1]) == 0, name
        assert torch.equal(gx[1], cs[1]) and torch.equal(gl[1], cw[1]), (name, gl[1].tolist(), cw[1].tolist())
    assert bool(torch.isfinite(gl[0]).all()) and bool(torch.isfinite(gl[2]).all()) and bool(torch.isfinite(gx[0]).all()), name


@pytest.mark.parametrize('name', list(special_cases()))
def test_special_rows(name):
    for dtype in (torch.float64, torch.float32):
        got = special_gradients(engine.sample_resample_tensor_ops, name, dtype)
        check_special_gradients(name, *got)
        # a NaN in the output gradient of the state reaches the row of its ancestor and nothing else
        out, gx, gl, cs, cw, cz = special_gradients(engine.sample_resample_tensor_ops, name, dtype, nan_row=2)
        parent = int(out.ancestor[0, 2])
        hit = torch.isnan(gx).reshape(-1, 3).any(dim=1).nonzero().flatten().tolist()
        assert hit == [parent], (name, hit, parent)
        assert torch.equal(gl, got[2]), name


def test_a_special_row_leaves_its_neighbours_gradients_alone():
    plain = special_gradients(engine.sample_resample_tensor_ops, 'a -Inf weight is never an ancestor', torch.float32)
    for name in ('a NaN', 'a +Inf', 'all -Inf', 'NaN beside -Inf'):
        got = special_gradients(engine.sample_resample_tensor_ops, name, torch.float32)
        for g in (0, 2):
            assert R_bits(got[1][g], plain[1][g]) and R_bits(got[2][g], plain[2][g]), (name, g)
