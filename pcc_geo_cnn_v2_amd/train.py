"""Training on the MI355X: the reference's `model.train` graph (src/model_types.py:250-277, :327-369) and `tr_train.py` loop.

Conv layers run as one torch.autograd.Function each over the library's kernels (forward: pcc_conv3d; backward: ReLU mask,
input gradient through the dual descriptor, weight / bias gradients through pcc_conv3d_wgrad).  The entropy models (tfc 1.3
semantics), residual adds, hyperprior wiring and the loss run in torch on the device.  The convs compute on a context of their own
whose exact-fp32 kernel families read only packed segments that pcc_conv_repack_weights_device rebuilds on the device after every
optimizer step (TRAIN_NUMERICS).
"""
import ctypes as C
import io
import json
import math
import os
import zipfile

import numpy as np
import torch

from . import _lib as L
from . import model_transforms as MT
from . import ops
from .utils import tf_summary

# The split (bf16 x 3), two-piece fp16 and Winograd kernels read packed images that are not reorders of the taps: off for training,
# so every conv runs an exact-fp32 family (conv_fwd, conv_tr2, conv_tr2m, conv_cin1, conv_cout1_mfma, conv_cout1) or the generic one.
TRAIN_NUMERICS = dict(no_split=True, no_f16s=True, no_winograd=True)
TAIL_MASS = 2 ** -8             # tfc 1.3 EntropyModel default (entropy_models.GaussianConditional)
LIKELIHOOD_BOUND = 1e-9


def training_context(device=None):
    """A context of its own (the inference contexts keep their kernel families) with TRAIN_NUMERICS set."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    ctx = ops.Context(device.index if device.index is not None else torch.cuda.current_device())
    ctx.set_numerics(**TRAIN_NUMERICS)
    return ctx


# ---------------------------------------------------------------------------------------------------------------------------------
# conv layers
# ---------------------------------------------------------------------------------------------------------------------------------
class TrainConv:
    """One Conv3D / Conv3DTranspose with device parameters; quacks like ops.ConvLayer for ops.conv3d."""

    def __init__(self, conv, device):
        l = conv.layer
        self.k, self.stride, self.transposed, self.relu = l.k, l.stride, l.transposed, l.relu
        self.cin, self.cout = l.cin, l.cout
        self.weight = torch.nn.Parameter(torch.from_numpy(l.kernel.copy()).to(device))
        self.bias_p = None if l.bias is None else torch.nn.Parameter(torch.from_numpy(l.bias.copy()).to(device))
        self.bias = l.bias          # presence only (ops.ConvLayer.desc)
        self._images = {}           # (grid, transposed) -> {'map', 'pk', 'ver'}

    def desc(self, N, D, H, W, flags=0, impl=L.PCC_IMPL_AUTO, out_cstride=0, out_coffset=0):
        return ops.ConvLayer.desc(self, N, D, H, W, flags, impl, out_cstride, out_coffset)

    def packed(self, ctx, d):
        """The packed image of descriptor d (the layer's or its dual) for the current weights, rebuilt on the device when the
        weights changed since (None: the generic kernel computes d)."""
        key = (d.D, d.H, d.W, d.transposed, d.Cin)
        im = self._images.get(key)
        if im is None:
            m = ops.conv_repack_map(d)
            im = self._images[key] = dict(map=None if m is None else torch.from_numpy(m).to(ctx.device), pk=None, ver=None)
            if m is not None:
                im['pk'] = torch.empty(m.shape, dtype=torch.float32, device=ctx.device)
        if im['map'] is not None and im['ver'] != self.weight._version:
            ops.conv_repack_device(ctx, d, im['map'], self.weight.detach(), im['pk'])
            im['ver'] = self.weight._version
        return im['pk']

    def device_images(self, ctx, d):
        return dict(w=self.weight.detach(), b=None if self.bias_p is None else self.bias_p.detach(), pk=self.packed(ctx, d))

    def parameters(self):
        return [self.weight] + ([] if self.bias_p is None else [self.bias_p])


class _ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, x, weight, bias, layer, pctx):
        x = x.contiguous()
        y = ops.conv3d(pctx, x, layer)
        fctx.layer, fctx.pctx = layer, pctx
        fctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(fctx, gy):
        x, y = fctx.saved_tensors
        layer, pctx = fctx.layer, fctx.pctx
        g = gy.contiguous().clone()
        if layer.relu:
            ops.relu_backward(pctx, g, y)                              # mask
        N, D, H, W, _ = x.shape
        d = layer.desc(N, D, H, W)
        dx = None
        dx = dgrad(pctx, layer, d, g, x) if fctx.needs_input_grad[0] else None
        dw = torch.empty_like(layer.weight)
        db = None if layer.bias_p is None else torch.empty_like(layer.bias_p)
        # one workspace per context: the backward calls run one after another on the context's stream
        ws = pctx.workspace(L.lib().pcc_conv_wgrad_workspace_bytes(C.byref(d)))
        ops.conv3d_wgrad(pctx, d, x, g, dw, db, ws)
        return dx, dw, db, None, None


def dgrad(pctx, layer, d, g, x):
    """Input gradient of layer descriptor d: pcc_conv3d on the dual descriptor with the same Keras array."""
    # a stride-2 Conv3D on an odd grid has no dual: a Conv3DTranspose writes 2 O voxels per axis, one more than x has
    assert d.transposed or d.stride == 1 or not (d.D | d.H | d.W) & 1, 'dgrad: stride-2 Conv3D on an odd grid'
    dd = ops.dual_desc(d)
    dx = torch.empty_like(x)
    L.check(L.lib().pcc_conv3d(pctx.handle, C.byref(dd), ops._ptr(g), ops._ptr(layer.weight.detach()),
                               ops._ptr(layer.packed(pctx, dd)), None, None, ops._ptr(dx), pctx.stream), 'pcc_conv3d (dgrad)')
    return dx


def conv(pctx, layer, x):
    return _ConvFn.apply(x, layer.weight, layer.bias_p, layer, pctx)


class _FocalFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, y_pred, y_true, gamma, alpha, pctx):
        y_pred, y_true = y_pred.contiguous(), y_true.contiguous()
        fctx.save_for_backward(y_pred, y_true)
        fctx.gamma, fctx.alpha, fctx.pctx = gamma, alpha, pctx
        return ops.focal_loss(pctx, y_true, y_pred, gamma, alpha)

    @staticmethod
    def backward(fctx, g):
        y_pred, y_true = fctx.saved_tensors
        scale = g.reshape(1).to(torch.float32).contiguous()
        return ops.focal_loss_grad(fctx.pctx, y_true, y_pred, scale, fctx.gamma, fctx.alpha), None, None, None, None


def focal_loss(pctx, y_true, y_pred, gamma=2.0, alpha=0.9):
    """src/utils/focal_loss.py:5-12 with its gradient (pcc_focal_loss / pcc_focal_loss_grad)."""
    return _FocalFn.apply(y_pred, y_true, float(gamma), float(alpha), pctx)


# ---------------------------------------------------------------------------------------------------------------------------------
# entropy models (tensorflow-compression 1.3 semantics)
# ---------------------------------------------------------------------------------------------------------------------------------
class _LowerBound(torch.autograd.Function):
    """tfc lower_bound: max(x, bound); the gradient passes where x >= bound or where it pushes x up (grad < 0)."""

    @staticmethod
    def forward(fctx, x, bound):
        fctx.save_for_backward(x)
        fctx.bound = bound
        return torch.clamp_min(x, bound)

    @staticmethod
    def backward(fctx, g):
        (x,) = fctx.saved_tensors
        return g * ((x >= fctx.bound) | (g < 0)).to(g.dtype), None


def lower_bound(x, bound):
    return _LowerBound.apply(x, float(bound))


class EntropyBottleneck:
    """Trainable factorized prior; parameters in the layout of entropy_models.EntropyBottleneck (export is a copy)."""

    def __init__(self, params, device, filters=(3, 3, 3)):
        self.filters = tuple(filters)
        self.params = {k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(device))
                       for k, v in params.items()}

    def density_parameters(self):
        return [v for k, v in self.params.items() if k != 'quantiles']

    def logits_cumulative(self, x, stop_gradient=False):
        """x: (C, 1, n) -> (C, 1, n)."""
        logits = x
        n = len(self.filters) + 1
        for i in range(n):
            m, b = self.params[f'matrix_{i}'], self.params[f'bias_{i}']
            if stop_gradient:
                m, b = m.detach(), b.detach()
            logits = torch.matmul(torch.nn.functional.softplus(m), logits) + b
            if i < n - 1:
                f = self.params[f'factor_{i}']
                f = f.detach() if stop_gradient else f
                logits = logits + torch.tanh(f) * torch.tanh(logits)
        return logits

    def __call__(self, y, noise):
        """y (N, ..., C) channels-last; noise: U(-1/2, 1/2) of y's shape.  Returns (y_tilde, likelihoods)."""
        C = y.shape[-1]
        y_tilde = y + noise
        v = y_tilde.reshape(-1, C).t().reshape(C, 1, -1)
        lower = self.logits_cumulative(v - .5)
        upper = self.logits_cumulative(v + .5)
        sign = -torch.sign(lower + upper).detach()
        lik = torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower))
        lik = lower_bound(lik, LIKELIHOOD_BOUND)
        return y_tilde, lik.reshape(C, -1).t().reshape(y.shape)

    def aux_loss(self):
        target = math.log(2 / TAIL_MASS - 1)
        t = torch.tensor([-target, 0., target], dtype=torch.float32, device=self.params['quantiles'].device)
        logits = self.logits_cumulative(self.params['quantiles'], stop_gradient=True)
        return torch.sum(torch.abs(logits - t))

    def numpy_params(self):
        return {k: v.detach().cpu().numpy().astype(np.float32) for k, v in self.params.items()}


def _std_cumulative(x):
    return .5 * torch.erfc(-(2 ** -.5) * x)


def gaussian_likelihood(y, sigma, noise, scale_bound=0.11):
    """tfc GaussianConditional (training): y_tilde = y + noise; Phi((1/2 - |y~|)/s) - Phi((-1/2 - |y~|)/s), s lower-bounded."""
    y_tilde = y + noise
    s = lower_bound(sigma, scale_bound)
    a = torch.abs(y_tilde)
    lik = _std_cumulative((.5 - a) / s) - _std_cumulative((-.5 - a) / s)
    return y_tilde, lower_bound(lik, LIKELIHOOD_BOUND)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model graph
# ---------------------------------------------------------------------------------------------------------------------------------
def _run(pctx, layer, x, convs):
    if isinstance(layer, MT._ConvBase):
        return conv(pctx, convs[id(layer)], x)
    if isinstance(layer, MT.ResidualLayer):
        t1 = _run(pctx, layer._layers[0], x, convs)
        t = t1
        for sub in layer._layers[1:]:
            t = _run(pctx, sub, t, convs)
        return t + t1 if layer.residual_mode == 'add' else torch.cat((t, t1), -1)
    for sub in layer._layers:
        x = _run(pctx, sub, x, convs)
    return x


class TrainGraph:
    """Parameters and loss of one model (CompressionModelV1 / V2) for training.  `model` must hold all its transforms (compress())."""

    def __init__(self, model, pctx):
        self.model, self.pctx = model, pctx
        self.v2 = hasattr(model, 'hyper_analysis_transform')
        dev = pctx.device
        self.convs = {}
        self.prefixed = []               # (prefix, index, TrainConv) in get_weights() order
        for prefix, tr, _ in model._transforms():
            for i, c in enumerate(tr.conv_layers()):
                tc = TrainConv(c, dev)
                self.convs[id(c)] = tc
                self.prefixed.append((prefix, i, tc))
        self.eb = EntropyBottleneck(model.entropy_bottleneck.params, dev, model.entropy_bottleneck.filters)
        self.scale_bound = float(model.scale_table[0]) if self.v2 else None

    def main_parameters(self):
        return [p for _, _, tc in self.prefixed for p in tc.parameters()] + self.eb.density_parameters()

    def aux_parameters(self):
        return [self.eb.params['quantiles']]

    def latent_shapes(self, x_shape):
        """Shapes of the noise tensors (y, and z for V2) for a batch x (N, D, H, W)."""
        N, D, H, W = x_shape
        F = self.model.num_filters
        y = (N, D // 8, H // 8, W // 8, F)
        return (y, (N, D // 16, H // 16, W // 16, F)) if self.v2 else (y,)

    def loss(self, x, noise, lmbda, gamma=2.0, alpha=0.9, tensors=False):
        """x (N, D, H, W) {0,1} float32 on the device; noise: tensors of latent_shapes(x.shape).  Returns dict of 0-d tensors:
        loss = lmbda * fl + mbpov (src/model_types.py:266-268 / :355-358), fl, mbpov.  tensors=True adds what summarize() reads:
        mbpov_y (V2: mbpov_z too; V1 reports mbpov as both mbpov/y and mbpov/total, src/model_types.py:270), num_occupied_voxels and
        `tensors`, the detached tensors of the reference's histogram summaries by tag."""
        m, pctx = self.model, self.pctx
        y = _run(pctx, m.analysis_transform, x.unsqueeze(-1), self.convs)
        num_occupied = torch.sum(x)
        denominator = -math.log(2) * num_occupied
        if self.v2:
            z = _run(pctx, m.hyper_analysis_transform, y, self.convs)
            z_tilde, z_lik = self.eb(z, noise[1])
            sigma = _run(pctx, m.hyper_synthesis_transform, z_tilde, self.convs)
            y_tilde, y_lik = gaussian_likelihood(y, sigma, noise[0], self.scale_bound)
            log_y, log_z = torch.log(y_lik), torch.log(z_lik)
            mbpov_y, mbpov_z = torch.sum(log_y) / denominator, torch.sum(log_z) / denominator
            mbpov = mbpov_y + mbpov_z
        else:
            y_tilde, y_lik = self.eb(y, noise[0])
            log_y = torch.log(y_lik)
            mbpov = mbpov_y = torch.sum(log_y) / denominator
        x_tilde = _run(pctx, m.synthesis_transform, y_tilde, self.convs)
        fl = focal_loss(pctx, x, x_tilde[..., 0], gamma, alpha)
        out = dict(loss=lmbda * fl + mbpov, fl=fl, mbpov=mbpov)
        if tensors:
            t = dict(y=y, y_tilde=y_tilde, x=x, x_tilde=x_tilde, y_likelihoods=y_lik, log_y_likelihoods=log_y)
            out.update(mbpov_y=mbpov_y.detach(), num_occupied_voxels=num_occupied.detach())
            if self.v2:
                t.update(z=z, z_tilde=z_tilde, sigma_tilde=sigma, z_likelihoods=z_lik, log_z_likelihoods=log_z)
                out['mbpov_z'] = mbpov_z.detach()
            out['tensors'] = {k: v.detach() for k, v in t.items()}
        return out

    def export_weights(self):
        """The checkpoint dictionary compress_octree / decompress_octree load (same keys as init_checkpoint): conv weights, the
        bottleneck's parameters and its CDF tables rebuilt from them (entropy_models.EntropyBottleneck._build)."""
        w = {}
        for prefix, i, tc in self.prefixed:
            w[f'{prefix}/{i}/kernel'] = tc.weight.detach().cpu().numpy()
            if tc.bias_p is not None:
                w[f'{prefix}/{i}/bias'] = tc.bias_p.detach().cpu().numpy()
        for k, v in self.eb.numpy_params().items():
            w[f'entropy_bottleneck/{k}'] = v
        self.model.set_weights(w)
        return self.model.get_weights()


# ---------------------------------------------------------------------------------------------------------------------------------
# summaries (src/model_types.py:65-105)
# ---------------------------------------------------------------------------------------------------------------------------------
V1_HISTOGRAMS = ('y', 'y_tilde', 'x', 'x_tilde', 'x_tilde_quant', 'y_likelihoods', 'log_y_likelihoods')
V2_HISTOGRAMS = ('z', 'z_tilde', 'sigma_tilde', 'z_likelihoods', 'log_z_likelihoods')
BC_TAGS = ('bc/precision', 'bc/recall', 'bc/accuracy', 'bc/specificity', 'bc/f1_score')


def binary_histogram(zeros, ones):
    """The histogram of a tensor that holds `zeros` 0.0 and `ones` 1.0 and nothing else (x_tilde_quant, from the confusion matrix:
    no pass over the tensor)."""
    limits = tf_summary.default_bucket_limits()
    counts = np.zeros(tf_summary.NUM_BUCKETS, np.uint64)
    b0, b1 = np.searchsorted(limits, [0.0, 1.0], side='right')
    counts[b0], counts[b1] = zeros, ones
    n = zeros + ones
    return dict(counts=counts, num=n, nonfinite=0, min=(0.0 if zeros else 1.0) if n else tf_summary.DBL_MAX,
                max=(1.0 if ones else 0.0) if n else -tf_summary.DBL_MAX, sum=float(ones), sum_squares=float(ones))


def binary_classification(tp, tn, fp, fn):
    """src/model_types.py:95-99 in float32; 0 / 0 is NaN, as TensorFlow's division gives."""
    tp, tn, fp, fn = (np.float32(v) for v in (tp, tn, fp, fn))
    with np.errstate(divide='ignore', invalid='ignore'):
        precision = tp / (tp + fp)
        recall = tp / (tp + fn)
        accuracy = (tp + tn) / (tp + tn + fp + fn)
        specificity = tn / (tn + fp)
        f1 = (np.float32(2) * precision * recall) / (precision + recall)
    return dict(zip(BC_TAGS, (float(v) for v in (precision, recall, accuracy, specificity, f1))))


def summarize(pctx, out):
    """{tag: float | histogram} of a TrainGraph.loss(..., tensors=True) result, tags and order of the reference's merged summary
    (v1_summaries, v2_summaries, binary_classification_summaries).  Histograms by pcc_tensor_histogram (one device-to-host copy for
    all of them), the scores from pcc_occupancy_scores; x_tilde_quant's histogram follows from the confusion matrix, its values
    being 0 and 1 only.  A tensor that holds NaN or Inf raises ValueError naming its tag (tf.summary.histogram fails there too)."""
    t = out['tensors']
    v2 = 'z' in t
    names = [k for k in V1_HISTOGRAMS + (V2_HISTOGRAMS if v2 else ()) if k != 'x_tilde_quant']
    hists = dict(zip(names, ops.tensor_histograms(pctx, [t[k] for k in names])))
    occ = ops.occupancy_scores(pctx, t['x'], t['x_tilde'])
    for k in names:
        if hists[k]['nonfinite']:
            raise ValueError(f"summary histogram '{k}': {hists[k]['nonfinite']} values are NaN or Inf")
    hists['x_tilde_quant'] = binary_histogram(occ['tn'] + occ['fn'], occ['tp'] + occ['fp'])
    num = lambda k: float(out[k].detach())
    s = {'loss': num('loss'), 'mbpov/y': num('mbpov_y'), 'mbpov/total': num('mbpov'), 'fl': num('fl'),
         'num_occupied_voxels': num('num_occupied_voxels')}
    s.update({k: hists[k] for k in V1_HISTOGRAMS})
    if v2:
        s.update({'z': hists['z'], 'z_tilde': hists['z_tilde'], 'mbpov/z': num('mbpov_z')})
        s.update({k: hists[k] for k in V2_HISTOGRAMS[2:]})
    s.update(binary_classification(occ['tp'], occ['tn'], occ['fp'], occ['fn']))
    return s


# ---------------------------------------------------------------------------------------------------------------------------------
# data, checkpoints, trainer
# ---------------------------------------------------------------------------------------------------------------------------------
def split_files(files):
    """src/tr_train.py:26-32: the parent directory's name, 'train' or 'test', decides."""
    cat = np.array([os.path.split(os.path.split(f)[0])[1] for f in files])
    files = np.asarray(files)
    return list(files[cat == 'train']), list(files[cat == 'test'])


def save_npz(path, arrays):
    """np.savez with fixed zip timestamps: the same arrays give the same bytes."""
    tmp = path + '.tmp'
    with zipfile.ZipFile(tmp, 'w', zipfile.ZIP_STORED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
    os.replace(tmp, path)


class Batches:
    """Seeded shuffled batches of point-cloud blocks, voxelised on the device; the order state is part of train_state.pt."""

    def __init__(self, blocks, batch_size, resolution, seed):
        assert len(blocks) > 0, 'no blocks'
        self.blocks, self.batch_size, self.resolution = blocks, int(batch_size), int(resolution)
        self.rng = np.random.default_rng(seed)
        self.order, self.pos = self.rng.permutation(len(blocks)), 0

    def next_indices(self):
        out = []
        while len(out) < self.batch_size:
            if self.pos == len(self.order):
                self.order, self.pos = self.rng.permutation(len(self.blocks)), 0
            out.append(int(self.order[self.pos]))
            self.pos += 1
        return out

    def dense(self, ctx, idx):
        R = self.resolution
        pts = [np.asarray(self.blocks[i])[:, :3] for i in idx]
        p = np.ascontiguousarray(np.concatenate(pts).astype(np.int32))
        assert p.size == 0 or (p.min() >= 0 and p.max() < R), f'block coordinates outside the {R}^3 grid'
        bof = np.concatenate([np.full(len(b), j, np.int32) for j, b in enumerate(pts)])
        return ops.voxelize(ctx, torch.from_numpy(p).to(ctx.device), torch.from_numpy(bof).to(ctx.device), len(idx), R, R, R)

    def next(self, ctx):
        return self.dense(ctx, self.next_indices())

    def state(self):
        return dict(rng=self.rng.bit_generator.state, order=self.order.tolist(), pos=self.pos)

    def load_state(self, s):
        self.rng.bit_generator.state = s['rng']
        self.order, self.pos = np.asarray(s['order']), int(s['pos'])


class Trainer:
    """src/tr_train.py's loop: Adam 1e-4 on lmbda * fl + mbpov, Adam 1e-3 on the bottleneck's aux loss, validation every
    `validation_interval` steps over `validation_steps` batches, model.npz on every new best validation loss, early stop after
    4 x the interval without improvement (saving the current model, as the reference does).

    train_state.pt (step, weights, both optimizers, noise generator, data order, best loss) is written atomically at every
    validation and at the end, so an interrupted run resumes from its last validation and replays the same steps.  A directory
    that holds a model.npz but no train_state.pt is refused: training there from scratch would overwrite that model.

    summary_interval N > 0 (the reference's value is 100; 0: off) writes TensorBoard event files where the reference does: the
    summary of every training step whose counter before the step is a multiple of N to <dir>/train/ under step + 1
    (src/tr_train.py:128,139-141), and one per validation batch i to <dir>/val/ under step + i (:104).  Every Trainer opens new
    event files.  Summaries draw no random numbers and touch no weights: model.npz and log.jsonl do not depend on N."""

    def __init__(self, model, checkpoint_dir, train_blocks, val_blocks, resolution=64, batch_size=32, lmbda=1e-4, alpha=0.9,
                 gamma=2.0, max_steps=100000, seed=42, validation_interval=500, validation_steps=10, warm_start=None,
                 device=None, log=print, summary_interval=0):
        self.model, self.dir = model, checkpoint_dir
        assert not (os.path.exists(os.path.join(checkpoint_dir, 'model.npz')) and not os.path.exists(self._state_path())), \
            f'{checkpoint_dir} holds a model.npz but no train_state.pt: not a training directory to resume (to start from that ' \
            'model, pass it as warm_start and train into another directory)'
        self.lmbda, self.alpha, self.gamma = float(lmbda), float(alpha), float(gamma)
        self.max_steps, self.seed = int(max_steps), int(seed)
        self.val_interval, self.val_steps = int(validation_interval), int(validation_steps)
        self.log = log
        self.summary_interval = int(summary_interval)
        assert self.summary_interval >= 0, 'summary_interval must be >= 0'
        self.pctx = training_context(device)
        R = int(resolution)
        if getattr(model, 'analysis_transform', None) is None:
            model.compress([1, 1, R, R, R])
        if warm_start:
            model.restore(warm_start)
        self.graph = TrainGraph(model, self.pctx)
        self.main_opt = torch.optim.Adam(self.graph.main_parameters(), lr=1e-4)
        self.aux_opt = torch.optim.Adam(self.graph.aux_parameters(), lr=1e-3)
        self.train_data = Batches(train_blocks, batch_size, R, seed)
        self.val_data = Batches(val_blocks, batch_size, R, seed + 1)
        self.gen = torch.Generator(device=self.pctx.device)
        self.gen.manual_seed(seed)
        self.step, self.best, self.best_step, self.last_val = 0, float('inf'), 0, None
        os.makedirs(checkpoint_dir, exist_ok=True)
        self.train_writer = self.val_writer = None
        if self.summary_interval:
            self.train_writer = tf_summary.EventFileWriter(os.path.join(checkpoint_dir, 'train'))
            self.val_writer = tf_summary.EventFileWriter(os.path.join(checkpoint_dir, 'val'))
        self._resume()

    def noise(self, x_shape, gen):
        return [torch.rand(s, generator=gen, device=self.pctx.device) - .5 for s in self.graph.latent_shapes(tuple(x_shape))]

    def train_step(self, x, tensors=False):
        out = self.graph.loss(x, self.noise(x.shape, self.gen), self.lmbda, self.gamma, self.alpha, tensors=tensors)
        aux = self.graph.eb.aux_loss()
        self.main_opt.zero_grad(set_to_none=True)
        self.aux_opt.zero_grad(set_to_none=True)
        out['loss'].backward()
        aux.backward()
        self.main_opt.step()
        self.aux_opt.step()
        out['aux'] = aux
        return out

    def validate(self):
        """Mean loss over validation_steps batches: a fixed batch sequence and fixed noise, so that validations compare."""
        data = Batches(self.val_data.blocks, self.val_data.batch_size, self.val_data.resolution, self.seed + 1)
        gen = torch.Generator(device=self.pctx.device)
        gen.manual_seed(self.seed + 2)
        tot = 0.
        with torch.no_grad():
            for i in range(self.val_steps):
                x = data.next(self.pctx)
                out = self.graph.loss(x, self.noise(x.shape, gen), self.lmbda, self.gamma, self.alpha,
                                      tensors=self.val_writer is not None)
                tot += float(out['loss'])
                if self.val_writer is not None:
                    self.val_writer.add_summary(summarize(self.pctx, out), self.step + i)
        return tot / self.val_steps

    # ---- checkpoint directory
    def _state_path(self):
        return os.path.join(self.dir, 'train_state.pt')

    def _save_model(self):
        save_npz(os.path.join(self.dir, 'model.npz'), self.graph.export_weights())

    def _save_state(self):
        params = {f'{p}/{i}/kernel': tc.weight.detach().cpu() for p, i, tc in self.graph.prefixed}
        params.update({f'{p}/{i}/bias': tc.bias_p.detach().cpu() for p, i, tc in self.graph.prefixed if tc.bias_p is not None})
        params.update({f'entropy_bottleneck/{k}': v.detach().cpu() for k, v in self.graph.eb.params.items()})
        tmp = self._state_path() + '.tmp'
        torch.save(dict(step=self.step, best=self.best, best_step=self.best_step, last_val=self.last_val, params=params,
                        main_opt=self.main_opt.state_dict(), aux_opt=self.aux_opt.state_dict(),
                        gen=self.gen.get_state(), train_data=self.train_data.state()), tmp)
        os.replace(tmp, self._state_path())

    def _resume(self):
        if not os.path.exists(self._state_path()):
            return
        s = torch.load(self._state_path(), map_location='cpu', weights_only=False)
        with torch.no_grad():
            for p, i, tc in self.graph.prefixed:
                tc.weight.copy_(s['params'][f'{p}/{i}/kernel'])
                if tc.bias_p is not None:
                    tc.bias_p.copy_(s['params'][f'{p}/{i}/bias'])
            for k, v in self.graph.eb.params.items():
                v.copy_(s['params'][f'entropy_bottleneck/{k}'])
        self.main_opt.load_state_dict(s['main_opt'])
        self.aux_opt.load_state_dict(s['aux_opt'])
        self.gen.set_state(s['gen'])
        self.train_data.load_state(s['train_data'])
        self.step, self.best, self.best_step = int(s['step']), float(s['best']), int(s['best_step'])
        self.last_val = s['last_val']

    def _log(self, rec):
        with open(os.path.join(self.dir, 'log.jsonl'), 'a') as f:
            f.write(json.dumps(rec) + '\n')
        if self.log:
            self.log(json.dumps(rec))

    def _validation(self):
        """Validate at this step; save model.npz on a new best and at early stop; always save the state.  True: stop."""
        v = self.validate()
        self.last_val = self.step
        self._log(dict(step=self.step, val_loss=v))
        stop = False
        if v < self.best:
            self.best, self.best_step = v, self.step
            self._save_model()
        elif self.step - self.best_step >= 4 * self.val_interval:
            self._save_model()            # src/tr_train.py:113-116: early stop saves the current model
            stop = True
        self._save_state()
        return stop

    def run(self):
        """Trains up to max_steps (resuming from train_state.pt), validating at every multiple of validation_interval (step 0
        and the last step included, each step once); writes the `done` marker at max_steps or early stop."""
        stopped = False
        while True:
            if self.step % self.val_interval == 0 and self.last_val != self.step and self._validation():
                stopped = True
                break
            if self.step >= self.max_steps:
                break
            x = self.train_data.next(self.pctx)
            get_summary = self.train_writer is not None and self.step % self.summary_interval == 0
            out = self.train_step(x, tensors=True) if get_summary else self.train_step(x)
            self.step += 1
            if get_summary:
                self.train_writer.add_summary(summarize(self.pctx, out), self.step)
            self._log(dict(step=self.step, fl=float(out['fl']), mbpov=float(out['mbpov']), loss=float(out['loss']),
                           aux=float(out['aux'])))
        self._save_state()
        if stopped or self.step >= self.max_steps:
            open(os.path.join(self.dir, 'done'), 'w').close()
        return self
