"""Float64 torch-CPU restatements for the training tests: the TF `SAME` convs of oracle/torch_oracle.py (same padding rules,
float64 instead of float32), the focal loss of src/utils/focal_loss.py, the tfc 1.3 entropy-model likelihoods and the whole
training loss of src/model_types.py:250-277 / :327-369."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def _same_pad(n, k, s):
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return tot // 2, tot - tot // 2


def conv3d(x, w, stride):
    """x (N,D,H,W,Cin), w (k,k,k,Cin,Cout), float64 tensors."""
    x = x.permute(0, 4, 1, 2, 3)
    w = w.permute(4, 3, 0, 1, 2)
    k = w.shape[2]
    p = [_same_pad(n, k, stride) for n in x.shape[2:]]
    x = F.pad(x, (p[2][0], p[2][1], p[1][0], p[1][1], p[0][0], p[0][1]))
    return F.conv3d(x, w, stride=stride).permute(0, 2, 3, 4, 1)


def conv3d_transpose(x, w, stride):
    """x (N,D,H,W,Cin), w (k,k,k,Cout,Cin): full transposed conv, cropped to [low, low + n*s)."""
    x = x.permute(0, 4, 1, 2, 3)
    w = w.permute(4, 3, 0, 1, 2)
    k = w.shape[2]
    y = F.conv_transpose3d(x, w, stride=stride)
    sl = []
    for n in x.shape[2:]:
        low, _ = _same_pad(n * stride, k, stride)
        sl.append(slice(low, low + n * stride))
    return y[:, :, sl[0], sl[1], sl[2]].permute(0, 2, 3, 4, 1)


def layer(x, w, b, stride, transposed, relu):
    y = (conv3d_transpose if transposed else conv3d)(x, w, stride)
    if b is not None:
        y = y + b
    return torch.relu(y) if relu else y


def focal_loss(y_true, y_pred, gamma=2.0, alpha=0.9):
    pt1 = torch.where(y_true == 1, y_pred, torch.ones_like(y_pred))
    pt0 = torch.where(y_true == 0, y_pred, torch.zeros_like(y_pred))
    lo, hi = float(np.float32(1e-3)), float(np.float32(.999))             # the float32 bounds the graph computes with
    pt1, pt0 = torch.clamp(pt1, lo, hi), torch.clamp(pt0, lo, hi)        # clamp's gradient passes at the bounds, like tf.clip_by_value
    return -torch.sum(alpha * (1 - pt1) ** gamma * torch.log(pt1)) - torch.sum((1 - alpha) * pt0 ** gamma * torch.log(1 - pt0))


def np_logits_cumulative(params, x, filters=(3, 3, 3)):
    """tfc 1.3 EntropyBottleneck._logits_cumulative in numpy float64; x (C, 1, n)."""
    logits = x
    for i in range(len(filters) + 1):
        m = np.logaddexp(0, params[f'matrix_{i}'].astype(np.float64))
        logits = m @ logits + params[f'bias_{i}']
        if i < len(filters):
            logits = logits + np.tanh(params[f'factor_{i}']) * np.tanh(logits)
    return logits


def np_eb_likelihood(params, v):
    """v (C, 1, n) -> likelihood with the sign trick, lower-bounded at 1e-9."""
    lo, up = np_logits_cumulative(params, v - .5), np_logits_cumulative(params, v + .5)
    s = -np.sign(lo + up)
    sig = lambda t: 1 / (1 + np.exp(-t))
    return np.maximum(np.abs(sig(s * up) - sig(s * lo)), 1e-9)


def np_gaussian_likelihood(v, sigma, bound=0.11):
    from scipy.stats import norm
    s = np.maximum(sigma, bound)
    a = np.abs(v)
    return np.maximum(norm.cdf((.5 - a) / s) - norm.cdf((-.5 - a) / s), 1e-9)


class _LB(torch.autograd.Function):
    """tfc lower_bound: max(x, b), gradient passed where x >= b or where it is negative (pushes x up)."""

    @staticmethod
    def forward(c, x, b):
        c.save_for_backward(x)
        c.b = b
        return torch.clamp_min(x, b)

    @staticmethod
    def backward(c, g):
        (x,) = c.saved_tensors
        return torch.where((x >= c.b) | (g < 0), g, torch.zeros_like(g)), None


def lower_bound(x, b):
    return _LB.apply(x, b)


def _eb64(params, y, filters=(3, 3, 3)):
    C = y.shape[-1]
    v = y.reshape(-1, C).t().reshape(C, 1, -1)

    def cum(x):
        for i in range(len(filters) + 1):
            x = torch.matmul(F.softplus(params[f'matrix_{i}']), x) + params[f'bias_{i}']
            if i < len(filters):
                x = x + torch.tanh(params[f'factor_{i}']) * torch.tanh(x)
        return x
    lo, up = cum(v - .5), cum(v + .5)
    s = -torch.sign(lo + up).detach()
    lik = torch.abs(torch.sigmoid(s * up) - torch.sigmoid(s * lo))
    return lower_bound(lik, 1e-9).reshape(C, -1).t().reshape(y.shape)


def model_loss64(graph, x, noise, lmbda, gamma=2.0, alpha=0.9):
    """The training loss of `graph` (pcc_geo_cnn_v2_amd.train.TrainGraph) restated in float64 on the CPU.  Returns
    (loss, aux, {name: leaf tensor}) with leaves named like the checkpoint keys."""
    import pcc_geo_cnn_v2_amd.model_transforms as MT
    leaves = {}
    for prefix, i, tc in graph.prefixed:
        leaves[f'{prefix}/{i}/kernel'] = tc.weight.detach().cpu().double().requires_grad_()
        if tc.bias_p is not None:
            leaves[f'{prefix}/{i}/bias'] = tc.bias_p.detach().cpu().double().requires_grad_()
    for k, v in graph.eb.params.items():
        leaves[f'entropy_bottleneck/{k}'] = v.detach().cpu().double().requires_grad_()
    key = {id(c): (p, i) for p, tr, _ in graph.model._transforms() for i, c in enumerate(tr.conv_layers())}

    def run(l, t):
        if isinstance(l, MT._ConvBase):
            p, i = key[id(l)]
            return layer(t, leaves[f'{p}/{i}/kernel'], leaves.get(f'{p}/{i}/bias'), l.stride, l.transposed, l.relu)
        if isinstance(l, MT.ResidualLayer):
            t1 = run(l._layers[0], t)
            u = t1
            for sub in l._layers[1:]:
                u = run(sub, u)
            return u + t1
        for sub in l._layers:
            t = run(sub, t)
        return t

    m = graph.model
    x = x.detach().cpu().double()
    noise = [n.detach().cpu().double() for n in noise]
    eb = {k.split('/', 1)[1]: v for k, v in leaves.items() if k.startswith('entropy_bottleneck/')}
    y = run(m.analysis_transform, x.unsqueeze(-1))
    den = -math.log(2) * torch.sum(x)
    if graph.v2:
        z = run(m.hyper_analysis_transform, y)
        z_t = z + noise[1]
        z_lik = _eb64(eb, z_t)
        sigma = run(m.hyper_synthesis_transform, z_t)
        y_t = y + noise[0]
        s = lower_bound(sigma, 0.11)
        a = torch.abs(y_t)
        cdf = lambda t: .5 * torch.erfc(-(2 ** -.5) * t)
        y_lik = lower_bound(cdf((.5 - a) / s) - cdf((-.5 - a) / s), 1e-9)
        mbpov = torch.sum(torch.log(y_lik)) / den + torch.sum(torch.log(z_lik)) / den
    else:
        y_t = y + noise[0]
        mbpov = torch.sum(torch.log(_eb64(eb, y_t))) / den
    x_t = run(m.synthesis_transform, y_t)
    loss = lmbda * focal_loss(x, x_t[..., 0], gamma, alpha) + mbpov
    target = math.log(2 / 2 ** -8 - 1)
    q = eb['quantiles']
    det = {k: v.detach() for k, v in eb.items()}
    lq = q
    for i in range(4):
        lq = torch.matmul(F.softplus(det[f'matrix_{i}']), lq) + det[f'bias_{i}']
        if i < 3:
            lq = lq + torch.tanh(det[f'factor_{i}']) * torch.tanh(lq)
    aux = torch.sum(torch.abs(lq - torch.tensor([-target, 0., target], dtype=torch.float64)))
    return loss, aux, leaves
