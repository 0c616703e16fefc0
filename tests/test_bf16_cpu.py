"""bf16 MFMA operands (options={'precision': 'bf16'}, SNSDE_FLAG_BF16_OPERANDS): the rounding of the numpy reference, the
option's refusals that need no GPU, and the host-side route queries of the library."""
import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.bf16_reference import round_bf16


def _torch_bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def test_round_bf16_matches_the_torch_cast():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    f = np.float32
    tie_lo = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0x00008000, 0x00018000, 0x7F7F8000, 0x7F7F7FFF], np.uint32).view(f)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 1.17e-38, 3.4028235e38, 1.0, -1.0, 0.1,
                        np.finfo(f).tiny, np.finfo(f).tiny / 3], f)
    snan = np.array([0x7F800001, 0xFF800001, 0x7FC00000, 0x7FBFFFFF, 0x7FFFFFFF], np.uint32).view(f)
    for v in (x, tie_lo, special, snan):
        got, want = round_bf16(v), _torch_bf16(v)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    # ties go to the even neighbour: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert round_bf16(np.array([1 + 2 ** -8, 1 + 3 * 2 ** -8], f)).tolist() == [1.0, 1 + 2 ** -6]


def test_path_name_and_flag():
    assert 'lean-bf16' in _lib.PATHS and _lib.PATHS.index('lean-bf16') == 9
    assert _lib.FLAG_BF16_OPERANDS == 16
    assert engine.precision_flags('fp32') == 0 and engine.precision_flags('bf16') == 16
    with pytest.raises(ValueError):
        engine.precision_flags('fp16')


def _k2(H=128, NL=2, io=4, no=17, C=21):
    return engine.model_struct(C, H, H, NL, io, no)


def test_routes_of_the_bf16_flag():
    """Host-side queries only: which configurations the bf16 kernel takes, and that the flag never routes to an f32 kernel."""
    assert engine.forward_path(_k2(), 1024, 101, 100) == 'lean'
    assert engine.forward_path(_k2(), 1024, 101, 100, precision='bf16') == 'lean-bf16'
    assert engine.forward_path(_k2(), 1024, 101, 100, 'milstein', precision='bf16') == 'lean-bf16'
    assert engine.forward_path(_k2(H=64, NL=3, io=1, no=3, C=5), 512, 21, 20, precision='bf16') == 'lean-bf16'
    # large batches: fp32 `auto` plans 16-row tiles, bf16 plans the 4-row tiles its kernel runs on
    assert engine.forward_path(_k2(), 16384, 101, 100) == 'mfma16'
    assert engine.forward_path(_k2(), 16384, 101, 100, precision='bf16') == 'lean-bf16'
    # not covered: SRK, H = 256 / 32, the diffusion nets, generic / 16-row kernels on request -> no kernel at all
    for m, kw in ((_k2(), dict(method='srk')), (_k2(H=256), {}), (_k2(H=32), {}), (_k2(no=18), {}),
                  (_k2(), dict(kernel='generic')), (_k2(), dict(kernel='mfma16'))):
        args = dict(method='euler', kernel='auto')
        args.update(kw)
        assert engine.forward_path(m, 1024, 101, 100, args['method'], args['kernel'], precision='bf16') == 'none', (m, kw)
        with pytest.raises(ValueError):
            engine.check_bf16(m, 1024, 101, 100, args['method'], args['kernel'])
    engine.check_bf16(_k2(), 1024, 101, 100)


def test_no_backward_for_bf16_descriptors():
    s = _lib.Solve()
    s.model = _k2()
    s.batch, s.knots, s.n_steps, s.n_out = 1024, 101, 100, 2
    s.method = _lib.EULER
    assert _lib.lib().snsde_backward_supported(C_ref(s)) == 1
    s.flags = _lib.FLAG_BF16_OPERANDS
    assert _lib.lib().snsde_backward_supported(C_ref(s)) == 0


def C_ref(s):
    import ctypes
    return ctypes.byref(s)


def _field(io=4, no=17, C=5, H=64, B=8, L=6):
    m = S.Diffusion_model(C, H, H, 2, input_option=io, noise_option=no)
    times = torch.arange(L, dtype=torch.float32)
    m.set_X(torch.zeros(B, L - 1, 4 * C), times)
    return m, torch.zeros(B, H), times


def test_sdeint_refuses_bf16_where_it_does_not_apply():
    m, y0, ts = _field()
    with pytest.raises(ValueError, match='precision'):
        S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'precision': 'fp16'})
    with pytest.raises(ValueError, match='torch'):
        S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'precision': 'bf16', 'backend': 'torch'})
    # under autograd: the field's parameters require grad (default), or y0 does
    with pytest.raises(ValueError, match='inference'):
        S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'precision': 'bf16'})
    with torch.no_grad():
        with pytest.raises(ValueError, match='CUDA'):
            S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'precision': 'bf16'})
    m.requires_grad_(False)
    with pytest.raises(ValueError, match='inference'):
        S.sdeint(m, y0.clone().requires_grad_(True), ts, dt=1.0, method='euler', options={'precision': 'bf16'})
    # the default and an explicit 'fp32' behave as before (CPU tensors: the tensor-op loop)
    with torch.no_grad():
        a = S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'seed': 3})
        b = S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'seed': 3, 'precision': 'fp32'})
    assert torch.equal(a, b)
