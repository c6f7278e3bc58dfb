"""The experiment YAML of tr_train_all, ev_run_experiment and ev_run_compare -- the schema of the reference's
src/ev_experiment.yml, and the directory layout its scripts share.

    EXPERIMENT_DIR/models/<checkpoint_id>/<lambda as %.2e>/        checkpoint directory (model.npz, done), + <lambda>.log
    EXPERIMENT_DIR/<pc_name>/<id>/<lambda>/                        ev_experiment's files of one (cloud, model, lambda)
    EXPERIMENT_DIR/<pc_name>/results/<eval_id>/                    ev_compare's files of one (cloud, eval mode)
    EXPERIMENT_DIR/results/                                        merged data.csv, bdrate.csv, bdsnr.csv, legends
    EXPERIMENT_DIR/gpcc/<mode id>/<pc_name>/**/report.json         G-PCC points (written by mp_report in the reference; here by ev_anchors)

Keys read (everything else in the file is ignored, PCERROR and MPEG_TMC13_DIR among them -- no external binary is run):

    EXPERIMENT_DIR, MPEG_DATASET_DIR (prefix of the data paths; optional)
    model_configs[]: id, config, lambdas, checkpoint_id (default: id), label, and opt_metrics / max_deltas / fixed_threshold /
                     alpha / gamma / batch_size / train_mode, each falling back to the top-level key of the same name
    data[]:          pc_name, input_pc, input_norm (optional), and the resolution of the cloud: `resolution:` is the size of the voxel
                     grid, what the CLIs' --resolution takes (1024 for a vox10 cloud); or `pcerror_cfg:` names a pc_error cfg
                     file, whose `resolution:` is the peak value (1023), one less; or, as in the reference, `cfg_name:` selects
                     MPEG_TMC13_DIR/cfg/<pcerror_mpeg_mode>/<cfg_name>/r06/pcerror.cfg
    eval_modes[]:    id, modes[] (id, label), lims, no_legend, rcParams
    bd_ignore, mpeg_modes[] (id, label)
    TRAIN_DATASET_PATH, TRAIN_RESOLUTION, alpha, gamma, batch_size, train_mode          (tr_train_all)
New, all optional: octree_level (top level or per cloud; default 4, the encoder's), estimate_normals, metrics_device, d2_ties,
consistency, no_merge_coding, recolor, codec_batch_size (top level): passed to ev_experiment.run_experiment (recolor, rank2 |
transfer, also picks the colour step of ev_run_anchor).  anchor_id, anchor_rates,
anchor_device: ev_run_anchor, which writes EXPERIMENT_DIR/gpcc/<anchor id>/ with this project's octree anchor codec (not G-PCC).
surface_anchor_id, surface_rates: ev_run_anchor --codec surface|both, the same tree from the surface anchor codec (not G-PCC, not
trisoup-conformant).
"""
import os

import yaml

TRAIN_MODES = ('independent', 'warm_seq')
OPT_GROUPS = ('d1', 'd2')


def load_experiment(path):
    with open(path) as f:
        exp = yaml.safe_load(f)
    assert isinstance(exp, dict), f'{path}: not a mapping'
    for key in ('EXPERIMENT_DIR', 'model_configs'):
        assert key in exp, f'{path}: {key} is missing'
    ids = [m['id'] for m in exp['model_configs']]
    assert len(set(ids)) == len(ids), f'{path}: duplicate model ids {ids}'
    return exp


def lmbda_to_str(lmbda):
    return f'{float(lmbda):.2e}'


def index_by_id(entries):
    return {e['id']: e for e in entries or ()}


def model_dir(exp, model_config, lmbda):
    """The checkpoint directory of one lambda of a model: `checkpoint_id` redirects it to another model's."""
    return os.path.join(exp['EXPERIMENT_DIR'], 'models', model_config.get('checkpoint_id', model_config['id']), lmbda_to_str(lmbda))


def model_log_path(exp, model_config, lmbda):
    return model_dir(exp, model_config, lmbda) + '.log'


def output_dir(exp, pc_name, model_config, lmbda):
    return os.path.join(exp['EXPERIMENT_DIR'], pc_name, model_config['id'], lmbda_to_str(lmbda))


def setting(exp, model_config, key, *default):
    """model_configs[].key, else the top-level key, else `default` (KeyError without one)."""
    if key in model_config:
        return model_config[key]
    if key in exp or not default:
        return exp[key]
    return default[0]


def coding_settings(exp, model_config):
    return dict(opt_metrics=list(setting(exp, model_config, 'opt_metrics')),
                max_deltas=[float(x) for x in setting(exp, model_config, 'max_deltas')],
                fixed_threshold=bool(setting(exp, model_config, 'fixed_threshold')))


def training_settings(exp, model_config):
    s = {k: setting(exp, model_config, k) for k in ('alpha', 'gamma', 'batch_size', 'train_mode')}
    assert s['train_mode'] in TRAIN_MODES, f"train_mode {s['train_mode']!r}: one of {TRAIN_MODES}"
    return s


def data_path(exp, rel):
    if rel is None:
        return None
    return os.path.join(exp.get('MPEG_DATASET_DIR') or '', rel)


def cloud_resolution(exp, entry):
    """Voxel grid size of one data[] entry (see the module docstring)."""
    if 'resolution' in entry:
        return int(entry['resolution'])
    cfg = entry.get('pcerror_cfg')
    if cfg is None and 'cfg_name' in entry and 'MPEG_TMC13_DIR' in exp and 'pcerror_mpeg_mode' in exp:
        cfg = os.path.join(exp['MPEG_TMC13_DIR'], 'cfg', exp['pcerror_mpeg_mode'], entry['cfg_name'], 'r06', 'pcerror.cfg')
    assert cfg is not None, f"data entry {entry.get('pc_name')}: needs resolution: or pcerror_cfg:"
    assert os.path.exists(cfg), f"{cfg} not found: give data entry {entry.get('pc_name')} a resolution: key"
    with open(cfg) as f:
        return int(yaml.safe_load(f)['resolution']) + 1


def opt_groups(opt_metrics):
    """The optimisation groups that a list of metrics produces files for: d1 always leads, d2 only with a d2_* metric."""
    return [g for g in OPT_GROUPS if any(m.startswith(g) for m in opt_metrics)]


def mode_label(exp, mode_id, eval_mode_entry):
    """Label of a mode of an eval set: its own, else the mpeg mode's / model's, else the id.  Unknown ids raise."""
    for table in (index_by_id(exp.get('mpeg_modes')), index_by_id(exp['model_configs'])):
        if mode_id in table:
            return eval_mode_entry.get('label', table[mode_id].get('label', mode_id))
    raise RuntimeError(f'Unknown mode {mode_id} {eval_mode_entry}')
