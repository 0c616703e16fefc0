"""torch restatement of the Diffusion_model solve under bf16 MFMA operands, differentiable: the arbiter of
options={'precision': 'bf16', 'bf16_grad': True} (SNSDE_FLAG_BF16_GRAD, include/snsde.h).

The forward is tests/bf16_reference.py: every matrix operand goes through q = round-to-nearest-even to bf16 - the weights (the
folded products emb . linear_in and emb . initial_network of input options 2 / 4 / 6 rounded as products) and the layer inputs
[sin t, cos t | y], X(t) and the hidden activations; everything else is the plain field.  In the backward pass q is the identity
(straight-through): for z = q(W) q(x) + b autograd then yields dL/dx = q(W)^T delta, dL/dW = delta (x) q(x), dL/db = sum delta, and
the gradient of a folded product flows on to emb, linear_in and initial_network through the unrounded product - the
specification of the fused backward.  Runs in the dtype of its parameters (float64: the arbiter; float32 on the CPU: the yardstick
of what float32 arithmetic alone does to these gradients).

The folded products.  The function the library differentiates rounds the FLOAT32 products its prepare launch forms
(csrc/snsde_mfma.hip: fold_block), and its backward rounds those same numbers.  tests/bf16_reference.py rounds the fp64 products
instead: of ~17 000 entries at H = 128 a few lie close enough to a bf16 rounding boundary to round the other way (measured on the
cases of tests/bf16_grad_cases.py: 0 - 4 entries), which is a neighbouring function - harmless to the states at 1e-4, but a weight
of typical size that differs by one bf16 ulp moves the gradient of EVERY row at first order (2-8-1-23-128-8-7-euler: entry 2.7e-2
of rms 2.1e-2, ten of 23 rows off by more than ROW_TOL).  folded='prepare' therefore takes the operand VALUES of the two folded
weights from `prepare_fold`, the prepare launch's float32 product restated operation for operation, and keeps everything else:
the gradient still flows through the product formed in the run's own dtype.  folded='fp64' is tests/bf16_reference.py's."""
import numpy as np
import torch

import stable_neural_sdes_amd as S
from oracle import sde_oracle as O


def round_bf16(x):
    """float32 tensor -> nearest bf16 (ties to even) as float32"""
    return x.to(torch.bfloat16).to(torch.float32)


def q(x):
    """an operand as the kernel multiplies it, with the identity as its derivative"""
    return x + (round_bf16(x.float()).to(x.dtype) - x).detach()


def prepare_fold(E, W):
    """F[f, k] = sum_j E[f, j] W[j, k] in float32 as the prepare launch forms it (fold_block): four fmaf chains over j = 0, 1, 2, 3
    mod 4, combined as (a0 + a1) + (a2 + a3).  (fmaf through float64: the product of two float32 is exact there, the sum is rounded
    twice - to float64, then to float32 - which differs from the single rounding only when the float64 sum falls exactly on a float32
    tie.)"""
    E, W = np.asarray(E, np.float32), np.asarray(W, np.float32)
    acc = [np.zeros((E.shape[0], W.shape[1]), np.float32) for _ in range(4)]
    for j in range(E.shape[1]):
        acc[j % 4] = (E[:, j:j + 1].astype(np.float64) * W[j:j + 1, :].astype(np.float64) + acc[j % 4].astype(np.float64)).astype(np.float32)
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


class Bf16GradField(torch.nn.Module):
    """f / g of a tests.helpers.make_problem dict with the operand rounding in the drift; usable as an `sde` of the package's
    tensor-op loop (options={'backend': 'torch'}) and by `solve` below."""
    sde_type, noise_type = 'ito', 'diagonal'

    def __init__(self, pr, dtype=torch.float64, rounded_products=False, folded='fp64'):
        """rounded_products (float32 runs): every matrix product is formed in float64 and rounded once to float32 - a second float32
        run of the same formulas whose roundings differ from the library GEMM's, for telling what float32 arithmetic as such does to
        a case from what one particular summation order does"""
        super().__init__()
        self.rounded_products = rounded_products
        self.qfold = None
        if folded == 'prepare' and pr['io'] in (2, 4, 6):      # the rounded operand values of the two folded weights (see above)
            E, H = np.asarray(pr['params']['emb.weight'], np.float32), pr['H']
            self.qfold = tuple(round_bf16(torch.from_numpy(prepare_fold(E[:, c:c + H], pr['params'][n]))).to(dtype)
                               for c, n in ((0, 'linear_in.weight'), (H, 'initial_network.weight')))
        elif folded not in ('fp64', 'prepare'):
            raise ValueError(folded)
        m = S.Diffusion_model(pr['C'], pr['H'], pr['H'], pr['NL'], input_option=pr['io'], noise_option=pr['no'])
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in pr['params'].items()})
        self.m = m.to(dtype)
        self.io, self.H = pr['io'], pr['H']
        self.coeffs = torch.from_numpy(pr['coeffs']).to(dtype)
        self.times_host = np.asarray(pr['times'], np.float32).astype(np.float64)

    def X(self, t):
        """oracle.spline_evaluate, operation for operation"""
        idx, frac = O.spline_index(self.times_host, float(t))
        frac = float(frac)
        C = self.coeffs.shape[-1] // 4
        row = self.coeffs[:, idx, :]
        a, b, two_c, three_d = (row[:, k * C:(k + 1) * C] for k in range(4))
        inner = 0.5 * two_c + three_d * frac / 3
        inner = b + inner * frac
        return a + inner * frac

    def _mm(self, x, W, Wq=None):
        """q(x) q(W)^T; Wq: the rounded values of W where they are not round_bf16(W) (a folded product, folded='prepare')"""
        W = q(W) if Wq is None else W + (Wq - W).detach()
        if self.rounded_products:
            return (q(x).double() @ W.double().T).to(x.dtype)
        return q(x) @ W.T

    def f(self, t, y):
        P, io, H = dict(self.m.named_parameters()), self.io, self.H
        mm = self._mm
        tau = self.m._tau(t, y)[1]
        Wi, bi = P['linear_in.weight'], P['linear_in.bias']
        if io == 0:
            z = mm(self.X(t), P['initial_network.weight']) + P['initial_network.bias']
        elif io in (1, 3, 5):
            inp = torch.cat([tau, y], dim=-1) if io in (3, 5) else y
            z = mm(inp, Wi) + bi
        else:
            E1, E2 = P['emb.weight'][:, :H], P['emb.weight'][:, H:]
            inp = torch.cat([tau, y], dim=-1) if io in (4, 6) else y
            qf = self.qfold or (None, None)
            z = (mm(inp, E1 @ Wi, qf[0]) + mm(self.X(t), E2 @ P['initial_network.weight'], qf[1])
                 + (P['emb.bias'] + E1 @ bi + E2 @ P['initial_network.bias']))
        z = z.relu()
        i = 0
        while f'linears.{i}.weight' in P:
            z = (mm(z, P[f'linears.{i}.weight']) + P[f'linears.{i}.bias']).relu()
            i += 1
        z = mm(z, P['linear_out.weight']) + P['linear_out.bias']
        if io in (5, 6):
            z = z * y.tanh()
        return z.tanh()

    def g(self, t, y):
        return self.m.g(t, y)


def solve(field, y0, ts, dt, dW, method='euler'):
    """oracle.integrate on tensors: the scheme on the float32 step grid of oracle.step_grid, Milstein's g dg/dy (dW^2 - h) as the
    vector-Jacobian product of the (elementwise) diffusion, differentiable."""
    t0s, t1s, out_step, w0, w1 = O.step_grid(np.asarray(ts, np.float32), dt)
    y, ys, k = y0, [y0], 0
    diff = torch.is_grad_enabled()
    for n in range(len(t0s)):
        t, h = float(t0s[n]), float(t1s[n]) - float(t0s[n])
        I, prev = dW[n], y
        if method == 'euler':
            y = y + field.f(t, y) * h + field.g(t, y) * I
        else:
            v = I * I - h
            with torch.enable_grad():
                yy = y if y.requires_grad else y.detach().requires_grad_(True)
                gv = field.g(t, yy)
                gdg = None
                if gv.requires_grad:
                    gdg, = torch.autograd.grad(gv, yy, grad_outputs=(gv if diff else gv.detach()) * v, allow_unused=True, create_graph=diff)
            gv = gv if diff else gv.detach()
            gdg = torch.zeros_like(y) if gdg is None else (gdg if diff else gdg.detach())
            y = y + field.f(t, y) * h + gv * I + 0.5 * gdg
        while k < len(out_step) and out_step[k] == n:
            ys.append(y if w0[k] == 0 else float(w0[k]) * prev + float(w1[k]) * y)
            k += 1
    return torch.stack(ys, 0)


def gradients(pr, ts, dt, dW, G, method='euler', dtype=torch.float64, rounded_products=False, folded='prepare'):
    """-> (ys, {'y0': dL/dy0, parameter name: gradient}) of L = (ys * G).sum() through `solve`, in `dtype` on the CPU."""
    field = Bf16GradField(pr, dtype, rounded_products, folded)
    y0 = torch.from_numpy(pr['y0']).to(dtype).requires_grad_(True)
    ys = solve(field, y0, ts, dt, torch.from_numpy(np.asarray(dW)).to(dtype), method)
    (ys * torch.as_tensor(G).to(dtype)).sum().backward()
    out = {'y0': y0.grad.detach()}
    for n, p in field.m.named_parameters():
        out[n] = torch.zeros_like(p) if p.grad is None else p.grad.detach()
    return ys.detach(), out
