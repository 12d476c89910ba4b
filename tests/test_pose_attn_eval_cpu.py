"""The one-call evaluation step of the cfg 003 head without a GPU: the C ABI (declared, exported, bound, refusing null
arguments before anything touches a device), which configurations deploy.FusedHeadEval takes and which it hands to the
module path (and why), the evaluation consumers of eval_utils, and the size of the float64 bounds
tests/test_pose_attn_eval_gpu.py asserts on the device (below 1 % of max |ref| for every case)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import yaml

import _ref_fixture as rf
from attentionalpoolingaction_amd import config as apa_config, deploy, eval_utils, nets_factory
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _pose_eval_ref as pe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('apa_pose_attn_eval_workspace_bytes', 'apa_pose_attn_eval_step')
P = 'USE_POSE_PRELOGITS_BASED_ATTENTION'


# ------------------------------------------------------------------------------------------ C ABI
def test_header_declares_library_exports_and_ctypes_binds_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'apa.h')).read()
    lib = cof.load_library()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, header), name + ' is not declared in include/apa.h'
        assert name in cof.exported_symbols()
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(cof._SIGNATURES[name][1])
    assert 'typedef struct apa_pose_attn_eval_io' in header
    # the ctypes structure follows the header's field order
    body = header[header.index('typedef struct apa_pose_attn_eval_io'):header.index('} apa_pose_attn_eval_io;')]
    fields = re.findall(r'(\w+);', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
    assert fields == [n for n, _ in cof.ApaPoseAttnEvalIO._fields_]


def test_workspace_size_covers_both_routes():
    lib = cof.load_library()
    N, Pn, C, Cp, J, K = 32, 196, 2048, 768, 16, 393
    for dt in (cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16):
        need = int(lib.apa_pose_attn_eval_workspace_bytes(N, Pn, C, Cp, J, K, 0, dt, 0))
        pose = int(lib.apa_pose_head_workspace_bytes(N, Pn, C, Cp, J, dt))
        pool = int(lib.apa_attn_pool_workspace_bytes(N, Pn, C, Cp, K, 1, 0))
        assert need >= pose + pool + (Cp // 128) * N * Pn * 4
        assert need == int(lib.apa_pose_attn_eval_workspace_bytes(N, Pn, C, Cp, J, K, 0, dt, 1))
    assert int(lib.apa_pose_attn_eval_workspace_bytes(0, Pn, C, Cp, J, K, 0, 0, 0)) == 0


def _io(**over):
    io = cof.ApaPoseAttnEvalIO()
    for n, _ in cof.ApaPoseAttnEvalIO._fields_[:19]:
        setattr(io, n, 256)                     # never dereferenced: every refusal below comes before the first launch
    io.W1_bf16 = io.labels = io.loss = io.Pl = None
    io.ws, io.ws_bytes, io.route = 256, 1 << 40, None
    for k, v in over.items():
        setattr(io, k, v)
    return io


REQUIRED = ('X', 'W1', 'b1', 'W2', 'b2', 'Wa', 'ba', 'Wt', 'bt', 'att', 'logits', 'zsave', 'abar', 'probs', 'pred')


@pytest.mark.parametrize('field', REQUIRED)
def test_null_required_pointer_is_refused(field):
    lib = cof.load_library()
    io = _io(**{field: None})
    rc = lib.apa_pose_attn_eval_step(ctypes.addressof(io), 2, 49, 64, 256, 16, 20, 0, cof.APA_DTYPE_BF16, None)
    assert rc == -1
    assert 'null' in lib.apa_last_error().decode()


def test_null_io_labels_without_loss_and_short_workspace():
    lib = cof.load_library()
    args = (2, 49, 64, 256, 16, 20, 0, cof.APA_DTYPE_BF16, None)
    assert lib.apa_pose_attn_eval_step(None, *args) == -1 and 'null' in lib.apa_last_error().decode()
    io = _io(labels=256)
    assert lib.apa_pose_attn_eval_step(ctypes.addressof(io), *args) == -1
    assert 'null' in lib.apa_last_error().decode()
    io = _io(ws_bytes=1024)
    assert lib.apa_pose_attn_eval_step(ctypes.addressof(io), *args) == -3
    assert 'workspace' in lib.apa_last_error().decode()
    io = _io()
    assert lib.apa_pose_attn_eval_step(ctypes.addressof(io), 2, 49, 64, 0, 16, 20, 0, cof.APA_DTYPE_BF16, None) == -1
    # channels that are no whole 16-byte vectors: refused before the pose head is launched
    assert lib.apa_pose_attn_eval_step(ctypes.addressof(io), 2, 49, 60, 256, 16, 20, 0, cof.APA_DTYPE_BF16, None) == -2


# ------------------------------------------------------------------------------------------ FusedHeadEval
def _cfg(net=None, train=None):
    apa_config.reset_cfg()
    return apa_config.cfg_from_dict({'NET': dict(net or {}), 'TRAIN': dict(train or {})})


def _build(cfg, is_training=False, **kw):
    return nets_factory.get_network_fn('resnet_v1_101', 20, 16, cfg, is_training=is_training, device='cpu',
                                       in_channels=32, **kw)


def _yaml_cfg(name, tmp_path, net_extra=None):
    path = rf.experiment_yaml(name, tmp_path)
    if net_extra:
        tree = yaml.safe_load(open(path))
        tree.setdefault('NET', {}).update(net_extra)
        path = os.path.join(str(tmp_path), 'variant_' + name)
        with open(path, 'w') as f:
            yaml.safe_dump(tree, f, default_flow_style=False)
    apa_config.reset_cfg()
    return apa_config.cfg_from_file(path)


@pytest.mark.parametrize('name,extra,pose_form', [
    ('002_MPII_ResNet_withAttention.yaml', None, False),
    ('003_MPII_ResNet_withPoseAttention.yaml', None, True),
    ('002_MPII_ResNet_withAttention.yaml', {P + '_PER_CLASS': True}, False),
], ids=['cfg002', 'cfg003', 'per_class_single_layer'])
def test_shipped_forms_are_taken(name, extra, pose_form, tmp_path):
    cfg = _yaml_cfg(name, tmp_path, extra)
    fn = _build(cfg)
    assert deploy.FusedHeadEval.unsupported_reason(fn.head, cfg, fn) == ''
    ev = deploy.FusedHeadEval(fn, cfg)
    assert ev.pose_form is pose_form and ev.multi_label is False
    if extra:
        assert fn.head.per_class and fn.head.single_layer
    apa_config.reset_cfg()


@pytest.mark.parametrize('net,kw,training,text', [
    ({P: True}, {}, True, 'training-mode'),
    ({'USE_POSE_ATTENTION_LOGITS': True}, {}, False, 'USE_POSE_ATTENTION_LOGITS'),
    ({}, {}, False, 'baseline'),
    ({P: True, P + '_RANK': 2}, {}, False, 'rank > 1'),
    ({P: True, P + '_WITH_POSE_FEAT': True, P + '_SINGLE_LAYER_ATT': True}, {}, False, '_WITH_POSE_FEAT'),
    ({P: True, P + '_SINGLE_LAYER_ATT': True}, {'want_topdown': True}, False, 'TopDownAttention'),
    ({P: True, P + '_PER_CLASS': True}, {}, False, 'per-class maps from pose_pre_logits'),
], ids=['training', 'pose_attention_logits', 'baseline', 'rank2', 'pose_feat', 'topdown', 'per_class_posepre'])
def test_refused_forms_name_their_reason(net, kw, training, text):
    cfg = _cfg(net)
    fn = _build(cfg, is_training=training, **kw)
    why = deploy.FusedHeadEval.unsupported_reason(fn.head, cfg, fn)
    assert why and text in why, why
    with pytest.raises(ValueError, match='FusedHeadEval'):
        deploy.FusedHeadEval(fn, cfg)
    apa_config.reset_cfg()


def test_multi_label_loss_selects_sigmoid_scores():
    cfg = _cfg({P: True}, {'LOSS_FN_ACTION': 'multi-label-2'})
    assert deploy.FusedHeadEval(_build(cfg), cfg).multi_label is True
    # FusedHeadStep's own refusals are what they were
    cfg = _cfg({P: True})
    fn = _build(cfg)
    assert 'training-mode' in deploy.FusedHeadStep.unsupported_reason(fn.head, cfg, fn)
    apa_config.reset_cfg()


# ------------------------------------------------------------------------------------------ eval_utils
def test_predict_multi_label_is_sigmoid_and_argmax_of_the_logits():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(9, 7, generator=g) * 3
    scores, pred = eval_utils.predict(logits, multi_label=True)
    want = 1.0 / (1.0 + np.exp(-logits.double().numpy()))
    assert scores.dtype == torch.float32 and np.abs(scores.numpy() - want).max() <= 4 * 2.0 ** -24
    assert torch.equal(pred, logits.argmax(1)) and pred.dtype == torch.int64
    import inspect
    assert inspect.signature(eval_utils.predict).parameters['multi_label'].default is False


def test_evaluation_accumulates_and_reports_through_compute_map_and_accuracy():
    rs = np.random.RandomState(11)
    scores = rs.rand(50, 7).astype(np.float32)
    labels = np.arange(50) % 7                       # every class present
    rs.shuffle(labels)
    scores[np.arange(50), labels] += 0.3 * (rs.rand(50) < 0.6)
    ev = eval_utils.Evaluation()
    for a, b in ((0, 16), (16, 17), (17, 50)):       # ragged batches
        ev.update(torch.from_numpy(scores[a:b]), torch.from_numpy(labels[a:b]))
    assert len(ev) == 50
    r = ev.result()
    m, aps = eval_utils.compute_map(scores, labels)
    assert r['mAP'] == m and r['aps'] == aps and len(aps) == 7
    assert r['accuracy'] == eval_utils.accuracy(scores, labels)
    assert 0.0 < r['accuracy'] < 1.0
    # the accumulated copies are the accumulator's own: a caller's buffer may be overwritten by the next batch
    buf = torch.from_numpy(scores[:10].copy())
    ev2 = eval_utils.Evaluation()
    ev2.update(buf, torch.from_numpy(labels[:10]).view(10, 1))
    buf.zero_()
    assert ev2.result()['accuracy'] == eval_utils.accuracy(scores[:10], labels[:10])
    with pytest.raises(ValueError):
        eval_utils.Evaluation().result()


# ------------------------------------------------------------------------------------------ the GPU test's bounds
@pytest.mark.parametrize('c', pe.CASES, ids=lambda c: c['name'])
def test_float64_bounds_are_below_one_percent(c):
    """What tests/test_pose_attn_eval_gpu.py asserts on the device holds for its inputs in float64: every stage bound
    is below 1 % of max |ref|, about half of the pose head's relu gates are open, and each image's largest logit
    leads by more than twice the logit bound."""
    inp = pe.make_inputs(c)
    att = pe.att_reference(c, inp)
    assert float(att.err.max()) < 0.01 * float(att.ref.abs().max())
    pre = inp['X'].double().reshape(-1, c['C']) @ inp['W1'].double() + inp['b1'].double()
    assert 0.25 <= float((pre > 0).double().mean()) <= 0.75
    if c['flags'] & pe.RELU_ATT:
        frac = float((att.ref > 0).double().mean())
        assert 0.2 <= frac <= 0.8, frac                 # the attention's relu gates both ways
    later = pe.later_reference(c, inp, att.ref.float())
    for k, b in later.items():
        assert float(b.err.max()) < 0.01 * float(b.ref.abs().max()), k
    gap, bnd = pe.top_two_gap(later['logits'])
    assert bool((gap > 2 * bnd).all())
    want = torch.tensor([(7 * n + 3) % c['K'] for n in range(c['N'])])
    assert torch.equal(later['logits'].ref.argmax(1), want)
