"""dL/dX of the spline coefficient constructions on the host: the three C entry points (exported, validated before any launch)
and the float64 restatement of the two transposes (tests/spline_grad_reference.py) against torch.autograd through the package's
tensor-op constructions.  No GPU compute.

The constructions are linear in the observed values, and everything else they compute depends on `times` and the NaN mask only,
so the restatement and autograd are the same linear map evaluated in float64: they agree to 1e-12 of the largest entry, and the
restatement writes exact zeros at missing entries.  That pins the specification the HIP kernels are tested against
(tests/test_gpu_spline_grad.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from stable_neural_sdes_amd import _lib
from tests import spline_grad_reference as R

NEW = ('snsde_spline_backward_workspace_bytes', 'snsde_natural_cubic_coeffs_backward', 'snsde_hermite_coeffs_backward')
ERR_NULL, ERR_DIMS, ERR_WORKSPACE = -1, -2, -5


def test_error_codes_are_the_header_s():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'snsde.h')).read()
    for name, code in (('SNSDE_ERR_NULL', ERR_NULL), ('SNSDE_ERR_DIMS', ERR_DIMS), ('SNSDE_ERR_WORKSPACE', ERR_WORKSPACE)):
        assert re.search(rf'{name}\s*=?\s*\(?{code}\b', hdr), name


def test_entry_points_are_in_exports_in_the_header_and_on_the_library():
    lib = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'snsde.h')).read()
    declared = set(re.findall(r'^SNSDE_API\s[^;(]*?\b(snsde_[a-z_0-9]+)\s*\(', hdr, re.M))
    for name in NEW:
        assert name in _lib.EXPORTS and name in declared and hasattr(lib, name), name
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) and set(_lib.EXPORTS) == declared
    assert lib.snsde_version() == 2
    assert lib.snsde_abi_check(2, C.sizeof(_lib.Model), C.sizeof(_lib.Solve), C.sizeof(_lib.Backward), C.sizeof(_lib.Head)) == 0


def test_entry_points_validate_before_they_touch_a_buffer():
    """Dummy non-null pointers: a call that got past its checks would launch a kernel on them (and, without a device, fail
    with the launch code instead of the one asserted here)."""
    lib = _lib.lib()
    p = C.c_void_p(4096)
    B, L, Cn = 7, 9, 21
    need = lib.snsde_spline_backward_workspace_bytes(B, L, Cn)
    assert need >= 4 * 4 * B * L * Cn                        # four [L][series] float planes
    assert lib.snsde_spline_backward_workspace_bytes(0, L, Cn) == 0 and lib.snsde_spline_backward_workspace_bytes(B, 1, Cn) == 0
    nat, her = lib.snsde_natural_cubic_coeffs_backward, lib.snsde_hermite_coeffs_backward
    for k in range(5):                                        # times, X, grad_coeffs, grad_X, workspace
        a = [p, p, p, p, p]
        a[k] = None
        assert nat(a[0], a[1], a[2], B, L, Cn, a[3], a[4], need, None) == ERR_NULL, k
        if k < 4:
            assert her(a[0], a[1], a[2], B, L, Cn, a[3], None) == ERR_NULL, k
    for dims in ((0, L, Cn), (-3, L, Cn), (B, 1, Cn), (B, 0, Cn), (B, L, 0)):
        assert nat(p, p, p, *dims, p, p, 1 << 40, None) == ERR_DIMS, dims
        assert her(p, p, p, *dims, p, None) == ERR_DIMS, dims
    assert nat(p, p, p, B, L, Cn, p, p, need - 1, None) == ERR_WORKSPACE
    assert nat(p, p, p, B, L, Cn, p, p, 0, None) == ERR_WORKSPACE


@pytest.mark.parametrize('key', R.CASE_KEYS, ids=lambda k: 'L%d-B%d-C%d' % k)
@pytest.mark.parametrize('kind', R.KINDS)
def test_restatement_is_the_transpose_autograd_computes(kind, key):
    c = R.case(*key)
    ref = R.autograd_gradient(kind, key).numpy()
    got = R.RESTATEMENT[kind](c['times'], c['X'], c['g'])
    assert got.shape == ref.shape == c['X'].shape and np.isfinite(got).all() and np.isfinite(ref).all()
    scale = np.abs(ref).max()
    assert scale > 0
    err = np.abs(got - ref).max() / scale
    print(f'{kind} {key}: restatement vs float64 autograd {err:.3e}')
    assert err <= 1e-12, err
    missing = np.isnan(c['X'])
    assert missing.any() and (got[missing] == 0.0).all() and (ref[missing] == 0.0).all()
    for (b, ch), name in c['planted'].items():
        if name == 'no observation':
            assert (got[b, :, ch] == 0.0).all(), (b, ch)
        elif name.startswith('one observation'):
            assert np.count_nonzero(got[b, :, ch]) <= 1, (b, ch)


def test_cases_hold_what_they_claim():
    c = R.case(9, 7, 21)
    assert len(c['planted']) == 24 and max(b * 21 + ch for b, ch in c['planted']) >= 128      # both workgroups
    obs = ~np.isnan(c['X'])
    names = {v: k for k, v in c['planted'].items()}
    b, ch = names['two observations at the ends (m == 2)']
    assert obs[b, :, ch].tolist() == [True] + [False] * 7 + [True]
    b, ch = names['no observation']
    assert not obs[b, :, ch].any()
    b, ch = names['one observation, interior']
    assert obs[b, :, ch].sum() == 1 and not obs[b, 0, ch] and not obs[b, -1, ch]
    frac = 1 - obs.mean()
    assert 0.2 < frac < 0.45, frac


def test_float32_input_on_the_cpu_keeps_the_tensor_op_route():
    """CPU tensors never meet the HIP Function: the gradient of a float32 CPU input is autograd's, close to float64's."""
    key = (9, 3, 5)
    g32, g64 = R.autograd_gradient('natural', key, torch.float32), R.autograd_gradient('natural', key)
    assert g32.dtype == torch.float32
    assert float((g32.double() - g64).abs().max()) / float(g64.abs().max()) < 1e-4
