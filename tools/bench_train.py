"""c3p training steps per second at batch 32 on 64^3 seeded blocks, and the same step with MIOpen convs (A/B).

    python tools/bench_train.py [--steps 20] [--warmup 3] [--batch_size 32] [--out profiles/train_bench.json]

HIP: train.TrainGraph as tr_train runs it (pcc_conv3d forward, dual-descriptor input gradients, pcc_conv3d_wgrad, device repack).
Device events split a HIP step into: conv forward (every pcc_conv3d of the transforms, the lazy device repack included), repack
(that repack alone; it runs inside conv forward and dgrad), entropy + loss forward (the rest of the forward), ReLU masks, dgrad, wgrad, the rest of the backward (entropy
models, loss, residual adds: torch autograd) and the optimizers.  The conv phases are sums of events around each call.
MIOpen: the same graph, entropy models, focal loss and optimizers with every conv replaced by torch.nn.functional.conv3d /
conv_transpose3d autograd in fp32 (TF SAME padding as oracle/torch_oracle.py) on contiguous NCDHW tensors: each layer copies its
NDHWC input to NCDHW and its output back, and those copies are inside the MIOpen time."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pcc_geo_cnn_v2_amd import train  # noqa: E402
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType  # noqa: E402


def seeded_blocks(n, res, seed=0):
    """Planes and shells, {0,1} float32 (n, res, res, res)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing='ij'), -1).astype(np.float32)
    out = np.zeros((n, res, res, res), np.float32)
    for i in range(n):
        if i % 2 == 0:
            nrm = rng.normal(size=3).astype(np.float32)
            nrm /= np.linalg.norm(nrm)
            out[i] = np.abs((g - res / 2) @ nrm - rng.uniform(-res / 6, res / 6)) < .6
        else:
            out[i] = np.abs(np.linalg.norm(g - res / 2, axis=-1) - rng.uniform(res / 5, res / 2.5)) < .6
    return out


def _pad(n, k, s):
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return tot // 2, tot - tot // 2


def miopen_conv(pctx, layer, x):
    """The layer through torch.nn.functional (MIOpen) autograd on contiguous NCDHW tensors, NDHWC in and out."""
    xc = x.permute(0, 4, 1, 2, 3).contiguous()
    k, s = layer.k, layer.stride
    w = layer.weight.permute(4, 3, 0, 1, 2).contiguous()
    if layer.transposed:
        y = F.conv_transpose3d(xc, w, stride=s)
        sl = [slice(_pad(n * s, k, s)[0], _pad(n * s, k, s)[0] + n * s) for n in xc.shape[2:]]
        y = y[:, :, sl[0], sl[1], sl[2]]
    else:
        p = [_pad(n, k, s) for n in xc.shape[2:]]
        y = F.conv3d(F.pad(xc, (p[2][0], p[2][1], p[1][0], p[1][1], p[0][0], p[0][1])), w, stride=s)
    if layer.bias_p is not None:
        y = y + layer.bias_p.view(1, -1, 1, 1, 1)
    if layer.relu:
        y = torch.relu(y)
    return _Contig.apply(y).permute(0, 2, 3, 4, 1).contiguous()


class _Contig(torch.autograd.Function):
    """Identity whose backward hands MIOpen a contiguous NCDHW gradient."""

    @staticmethod
    def forward(ctx, y):
        return y

    @staticmethod
    def backward(ctx, g):
        return g.contiguous()


class Phases:
    """Device events around the library calls of a step, summed per phase."""
    NAMES = ('conv_fwd', 'repack', 'relu_mask', 'dgrad', 'wgrad')

    def __init__(self):
        self.events = {n: [] for n in self.NAMES}
        self._orig = {}

    def _wrap(self, mod, attr, name):
        f = getattr(mod, attr)
        self._orig[(mod, attr)] = f

        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = f(*a, **k)
            e1.record()
            self.events[name].append((e0, e1))
            return r
        setattr(mod, attr, timed)

    def install(self):
        self._wrap(train.ops, 'conv3d', 'conv_fwd')
        self._wrap(train.ops, 'conv_repack_device', 'repack')
        self._wrap(train.ops, 'relu_backward', 'relu_mask')
        self._wrap(train, 'dgrad', 'dgrad')
        self._wrap(train.ops, 'conv3d_wgrad', 'wgrad')

    def remove(self):
        for (mod, attr), f in self._orig.items():
            setattr(mod, attr, f)

    def take(self):
        out = {n: sum(a.elapsed_time(b) for a, b in v) for n, v in self.events.items()}
        self.events = {n: [] for n in self.NAMES}
        return out


def run(graph, x, noise, steps, warmup, phases=None):
    opt = torch.optim.Adam(graph.main_parameters(), lr=1e-4)
    aux_opt = torch.optim.Adam(graph.aux_parameters(), lr=1e-3)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    times, split = [], []
    for i in range(warmup + steps):
        e = [ev() for _ in range(4)]
        e[0].record()
        out = graph.loss(x, noise, 1e-4)
        aux = graph.eb.aux_loss()
        e[1].record()
        opt.zero_grad(set_to_none=True)
        aux_opt.zero_grad(set_to_none=True)
        (out['loss'] + aux).backward()
        e[2].record()
        opt.step()
        aux_opt.step()
        e[3].record()
        torch.cuda.synchronize()
        p = phases.take() if phases else None
        if i >= warmup:
            times.append([e[j].elapsed_time(e[j + 1]) for j in range(3)])
            if p:
                split.append(p)
    t = np.median(np.array(times), axis=0)
    res = dict(step_ms=float(sum(t)), forward_ms=float(t[0]), backward_ms=float(t[1]), optimizer_ms=float(t[2]),
               steps_per_s=float(1000.0 / sum(t)))
    if split:
        m = {n: float(np.median([p[n] for p in split])) for n in Phases.NAMES}
        m['entropy_loss_fwd'] = res['forward_ms'] - m['conv_fwd']
        m['rest_of_backward'] = res['backward_ms'] - m['relu_mask'] - m['dgrad'] - m['wgrad']
        res['phases_ms'] = m
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch_size', type=int, default=32)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--no_miopen', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    pctx = train.training_context(torch.device('cuda', 0))
    R = a.resolution
    model = ModelConfigType['c3p'].build(seed=42)
    model.compress([1, 1, R, R, R])
    graph = train.TrainGraph(model, pctx)
    x = torch.from_numpy(seeded_blocks(a.batch_size, R)).cuda()
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    noise = [torch.rand(s, generator=gen, device='cuda') - .5 for s in graph.latent_shapes(tuple(x.shape))]
    res = dict(model='c3p', batch_size=a.batch_size, resolution=R, device=torch.cuda.get_device_name(0))
    res['hip'] = run(graph, x, noise, a.steps, a.warmup)
    ph = Phases()
    ph.install()
    try:
        res['hip_phases'] = run(graph, x, noise, a.steps, a.warmup, ph)
    finally:
        ph.remove()
    if not a.no_miopen:
        hip_conv = train.conv
        train.conv = miopen_conv
        try:
            ref = ModelConfigType['c3p'].build(seed=42)
            ref.compress([1, 1, R, R, R])
            res['miopen'] = run(train.TrainGraph(ref, pctx), x, noise, a.steps, a.warmup)
        finally:
            train.conv = hip_conv
        res['hip_over_miopen'] = res['hip']['steps_per_s'] / res['miopen']['steps_per_s']
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
