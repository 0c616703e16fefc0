"""numpy fp64 restatement of the drift under bf16 MFMA operands (SNSDE_FLAG_BF16_OPERANDS, csrc/snsde_m4b_kernel.h).

The kernel rounds exactly two things to bf16 (round to nearest even): the weights of every layer the MFMAs multiply and the
layer inputs it writes to LDS ([X(t) | sin t, cos t], y, the hidden activations).  Products are summed in f32 there and in fp64
here; everything else (biases, relu, tanh, the diffusion, the increments, the update, the output interpolation) is
oracle/sde_oracle.py unchanged.  The embedded input options (2, 4, 6) run with the first two layers pre-multiplied
(SNSDE_FLAG_EXACT_ORDER clear): emb o linear_in and emb o initial_network are ONE layer whose weights are the products, so those
products are what is rounded (formed in fp64 here, in f32 by the prepare launch: an operand next to a tie may round the other way).
"""
import numpy as np

from oracle import sde_oracle as O


def round_bf16(x):
    """float32 -> nearest bf16 (ties to even), returned as float32; NaN stays NaN, +-inf and overflow to +-inf as in the cast."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    r = np.where(np.isnan(x), (u | 0x400000) & 0xFFFF0000, r)      # (quiet NaN, sign kept)
    return (r.astype(np.uint32)).view(np.float32).reshape(x.shape)


def _q(x):
    """an operand as the kernel sees it: the f32 value, rounded to bf16, widened to fp64"""
    return round_bf16(np.asarray(x, dtype=np.float64).astype(np.float32)).astype(np.float64)


def drift_f_bf16(p, io, t, y, Xt_raw):
    """oracle.drift_f with bf16 operands (p: fp64 parameter dict)."""
    B = y.shape[0]
    _, tf = O.time_features(t, B, np.float64)
    Wi, bi = p['linear_in.weight'], p['linear_in.bias']
    if io == 0:
        z = _q(Xt_raw) @ _q(p['initial_network.weight']).T + p['initial_network.bias']
    elif io in (1, 3, 5):
        inp = np.concatenate([tf, y], axis=-1) if io in (3, 5) else y
        z = _q(inp) @ _q(Wi).T + bi
    else:                  # folded: z = (E1 W_in) [tf | y] + (E2 W_init) X + (b_emb + E1 b_in + E2 b_init)
        H = y.shape[1]
        E1, E2 = p['emb.weight'][:, :H], p['emb.weight'][:, H:]
        inp = np.concatenate([tf, y], axis=-1) if io in (4, 6) else y
        z = (_q(inp) @ _q(E1 @ Wi).T + _q(Xt_raw) @ _q(E2 @ p['initial_network.weight']).T
             + (p['emb.bias'] + E1 @ bi + E2 @ p['initial_network.bias']))
    z = np.maximum(z, 0)
    i = 0
    while f'linears.{i}.weight' in p:
        z = np.maximum(_q(z) @ _q(p[f'linears.{i}.weight']).T + p[f'linears.{i}.bias'], 0)
        i += 1
    z = _q(z) @ _q(p['linear_out.weight']).T + p['linear_out.bias']
    if io in (5, 6):
        z = z * np.tanh(y)
    return np.tanh(z)


def solve_bf16(p, io, no, coeffs, times, y0, ts, dt, dW, method='euler'):
    """oracle.solve_diffusion_model (fp64) with the bf16-operand drift."""
    p = O.cast_params(p, np.float64)
    coeffs = np.asarray(coeffs, dtype=np.float64)
    times_d = np.asarray(times, dtype=np.float32).astype(np.float64)

    def f(t, y):
        return drift_f_bf16(p, io, t, y, O.spline_evaluate(coeffs, times_d, t))

    def g(t, y):
        return O.diffusion_g(p, no, t, y)

    def gdg(t, y):
        return O.diffusion_g_dgdy(p, no, t, y)

    return O.integrate(f, g, np.asarray(y0, dtype=np.float64), ts, dt, np.asarray(dW), method=method, gdg=gdg)
