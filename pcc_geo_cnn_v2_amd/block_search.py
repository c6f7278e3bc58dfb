"""How the adaptive per-block threshold search (model_opt.py) is scheduled around the encoder's chunks: `search_plan` states which
engine computes what, `SearchSchedule` queues the work of each chunk and takes the decisions a few chunks later."""
import os
from collections import namedtuple

import numpy as np

from .model_opt import d1_tallies_gpu, d12_tallies_gpu, d2_on_gpu, decide_from_tallies, gpu_search_supported, metric_names
from .utils.pc_metric import wants_hausdorff

# gpu_tallies: None | 'd1' (d1_tallies_gpu) | 'd12' (d12_tallies_gpu);  host_job: None or the HostSearchPool job kind of every block;
# ties: the rule of the D2 statistics ('pick' when no d2_* metric is asked for)
SearchPlan = namedtuple('SearchPlan', 'gpu_tallies host_job ties')


def search_plan(opt_metrics, dhw, ties='pick', d2_gpu=False, no_prune=False):
    """The engines of the adaptive search (model_opt.py:33-73) for one metric list and grid.

        grid above 128^3                    no GPU tallies, 'decide' jobs: the whole decision per block in the host pool
        d1_* metrics only                   'd1' tallies, no host jobs
        d2_*, statistics from the GPU       'd12' tallies, no host jobs (d2_gpu: model_opt.d2_on_gpu)
        d2_*, KD-trees, ties 'pick'         'd1' tallies FIRST: they bound the 'tally_pruned' jobs, which only build the A->B trees of
                                            the thresholds that can still win a d2 metric (model_opt.host_threshold_stats_pruned)
        the same with no_prune, or 'mean'   'tally' jobs: every level set (PCC_D2_NO_PRUNE=1: A/B runs; 'mean' with KD-trees is
                                            the host restatement, for checking), merged with the 'd1' tallies

    d1_* metrics: exact distance transforms on the GPU, with or without normals in the input.  d2_* metrics: the reference's numbers
    depend on WHICH of several equidistant nearest neighbours scipy's KD-tree returns (measured: another tie rule moves d2_mse by
    up to 60 % and the chosen threshold in 2 of 6 blocks), so by default those tallies come from the same KD-trees on the host."""
    want_d2 = any(m.startswith('d2_') for m in opt_metrics)
    ties = ties if want_d2 else 'pick'
    if not gpu_search_supported(opt_metrics, dhw):
        return SearchPlan(None, 'decide', ties)
    if not want_d2:
        return SearchPlan('d1', None, ties)
    if d2_gpu:
        return SearchPlan('d12', None, ties)
    return SearchPlan('d1', 'tally_pruned' if ties == 'pick' and not no_prune else 'tally', ties)


class SearchSchedule:
    """The adaptive search of one encode_block_range call.  add(chunk, x_hat) enqueues a chunk's GPU tallies and only QUEUES its
    host jobs -- one block per worker process of a persistent pool (the reference runs the blocks one after the other); the GPU goes
    on with the next chunks and the decisions are taken (on the merged table) SEARCH_LAG chunks later, so the pool always holds
    several chunks' worth of blocks.  drain() takes the remaining ones.  Results: `thresholds` (best index per metric, per block),
    `points` (candidate point lists per metric, per block), `names`."""
    SEARCH_LAG = 8            # chunks whose x_hat (batch x 1 MiB) stays on the GPU while their host jobs are in the pool

    def __init__(self, model, ctx, dhw, n_blocks, resolution, with_normals, opt_metrics, max_deltas):
        self.model, self.ctx, self.dhw, self.n_blocks = model, ctx, tuple(dhw), n_blocks
        self.resolution, self.with_normals = resolution, with_normals
        self.opt_metrics, self.max_deltas = opt_metrics, max_deltas
        self.plan = None
        self.pending, self.thresholds, self.points = [], [], []
        self.names = metric_names(opt_metrics, max_deltas)

    def _make_plan(self):
        m, dhw = self.model, self.dhw
        want_d2 = any(name.startswith('d2_') for name in self.opt_metrics)
        # search_ties 'mean' (DESIGN.md 4.6): the tie-averaged d2 statistics, the same sums on either engine -- from the GPU unless
        # d2_search = 'kdtree' asks for the host restatement.  'pick': nearest-index transforms, stated tie rule: opt-in (DESIGN_HISTORY.md 3.8)
        ties = m.search_ties if want_d2 else 'pick'
        d2_gpu = want_d2 and gpu_search_supported(self.opt_metrics, dhw) and d2_on_gpu(m.d2_search, ties)
        return search_plan(self.opt_metrics, dhw, ties, d2_gpu, bool(os.environ.get('PCC_D2_NO_PRUNE')))

    def _jobs(self, kind, chunk, xh, d1):
        # blocks go over in their own dtype: the worker computes exactly what the in-process call would
        thr, wn, ties = self.model.thresholds, self.with_normals, self.plan.ties
        blocks = [np.ascontiguousarray(b) for b in chunk]
        if kind == 'tally_pruned':
            return [(kind, b, xh[j], thr, wn, d1[j][:, :5], self.resolution, list(self.opt_metrics), list(self.max_deltas)) for j, b in enumerate(blocks)]
        if kind == 'tally':
            return [(kind, b, xh[j], thr, wn, ties) for j, b in enumerate(blocks)]
        return [(kind, b, xh[j], thr, self.resolution, wn, list(self.opt_metrics), list(self.max_deltas), ties) for j, b in enumerate(blocks)]

    def add(self, chunk, x_hat):
        m, ctx = self.model, self.ctx
        if self.plan is None:
            self.plan = self._make_plan()      # (with the first chunk: d2_on_gpu logs what it chose)
        plan = self.plan
        item = dict(chunk=chunk, x_hat=x_hat, futures=None, d1=None)
        hd = wants_hausdorff(self.opt_metrics)      # 9-slot tallies: the Hausdorff forms of the GPU calls, made only then
        if plan.host_job == 'tally_pruned':         # (the pruned jobs bound sums: they get the five sum slots)
            item['d1'] = d1_tallies_gpu(ctx, chunk, x_hat, m.thresholds, hausdorff=hd)
        if plan.host_job is not None:
            jobs = self._jobs(plan.host_job, chunk, np.clip(x_hat.cpu().numpy(), 0.0, 1.0), item['d1'])
            m.host_search_jobs += len(jobs)
            m.last_host_job_kind = jobs[0][0] if jobs else None
            pool = m._search_pool(self.n_blocks)
            item['futures'] = [pool.submit(job) for job in jobs]
        if plan.gpu_tallies is not None and item['d1'] is None:
            item['d1'] = d12_tallies_gpu(ctx, chunk, x_hat, m.thresholds, ties=plan.ties, hausdorff=hd) if plan.gpu_tallies == 'd12' \
                else d1_tallies_gpu(ctx, chunk, x_hat, m.thresholds, hausdorff=hd)
        self.pending.append(item)
        if len(self.pending) > self.SEARCH_LAG:
            self._finalize(self.pending.pop(0))

    def drain(self):
        while self.pending:
            self._finalize(self.pending.pop(0))

    def _finalize(self, item):
        """decisions + candidate point lists of one chunk whose tallies (GPU) / host results are complete"""
        m, plan = self.model, self.plan
        chunk, x_hat = item['chunk'], item['x_hat']
        n_m = len(self.max_deltas) * len(self.opt_metrics)
        host = [f.result() for f in item['futures']] if item['futures'] is not None else None
        if plan.host_job == 'tally_pruned':      # (tallies, (mean_tally, thresholds evaluated exactly)) per block
            m.search_trees_built += sum(h[1][1] for h in host)
            m.search_trees_total += sum(len(h[0]) for h in host)
            host = [(h[0], h[1][0]) for h in host]
        if item['d1'] is not None:
            self.names, best_all = decide_from_tallies(chunk, item['d1'], len(m.thresholds), self.resolution, self.opt_metrics, self.max_deltas,
                                                       host, gpu_d2=plan.gpu_tallies == 'd12', ties=plan.ties)
        else:
            self.names, best_all = host[0][0], [bt for _, bt in host]
        # a block whose decode is empty at every threshold returns len(opt_metrics) entries (model_opt.py:35-36); with
        # more than one max_delta the reference's zip(*...) would silently drop the other candidates of the WHOLE
        # cloud -- here the 'emit nothing' index is repeated instead
        best_all = [list(bt) + [bt[-1]] * (n_m - len(bt)) for bt in best_all]
        per_metric = []
        for k in range(n_m):
            xyz, counts = m._extract_points(self.ctx, x_hat, [bt[k] for bt in best_all], clip=True)
            per_metric.append(m._gather_points(xyz, counts))
        for j in range(len(chunk)):
            self.thresholds.append(list(best_all[j]))
            self.points.append([per_metric[k][j] for k in range(n_m)])
