"""deploy.HeadSweep without a GPU: the stacking makes views (a row written through the stack is seen by its head and the
other way round, state_dict() still works), and heads that differ are refused by the name of the difference."""
import os

import pytest
import torch

import _ref_fixture as rf
from attentionalpoolingaction_amd import config as apa_config, deploy

TRAIN_FX = os.path.join(rf.GOLD, 'ref_head_cfg002_train_c2048_libmask.npz')


def _heads(n, **kw):
    fx = rf.HeadFixture(TRAIN_FX)
    fns, cfg = [], None
    for i in range(n):
        torch.manual_seed(i)
        fn, cfg = rf.build_head(fx, device='cpu', **kw)
        fns.append(fn)
    return fns, cfg


def test_stacking_makes_views_both_ways():
    try:
        fns, cfg = _heads(3)
        before = [{k: v.clone() for k, v in fn.head.state_dict().items() if isinstance(v, torch.Tensor)} for fn in fns]
        sweep = deploy.HeadSweep(fns, cfg, lrs=[0.1, 0.01, 0.001])
        H, C, K = 3, sweep.C, sweep.K
        assert tuple(sweep.Wa.shape) == (H, C) and tuple(sweep.ba.shape) == (H,)
        assert tuple(sweep.Wt.shape) == (H, C, K) and tuple(sweep.bt.shape) == (H, K)
        for h, fn in enumerate(fns):
            sd = fn.head.state_dict()
            for k, v in before[h].items():                       # nothing moved
                assert torch.equal(sd[k], v), (h, k)
            assert fn.head.td_weights.data_ptr() == sweep.Wt[h].data_ptr()
            assert fn.head.att_weights.data_ptr() == sweep.Wa[h].data_ptr()
        with torch.no_grad():
            sweep.Wt[1].fill_(0.25)                              # through the stack ...
            fns[2].head.att_biases.fill_(-3.0)                   # ... and through a head
            fns[0].head.td_biases[4] = 7.0
        assert float(fns[1].head.td_weights.min()) == float(fns[1].head.td_weights.max()) == 0.25
        assert float(fns[0].head.td_weights.abs().max()) != 0.25
        assert float(sweep.ba[2]) == -3.0 and float(sweep.ba[0]) != -3.0
        assert float(sweep.bt[0, 4]) == 7.0
        assert float(fns[1].head.state_dict()['td_weights'].max()) == 0.25
        assert sweep.weight_decays == [float(fn.weight_decay) for fn in fns]
    finally:
        apa_config.reset_cfg()


def test_mismatched_heads_are_refused_by_name():
    try:
        fns, cfg = _heads(2)
        fns[1].head.relu_att = not fns[0].head.relu_att
        with pytest.raises(ValueError, match='head 1 differs from head 0 in relu_att'):
            deploy.HeadSweep(fns, cfg, lrs=[0.1, 0.1])
        fns, cfg = _heads(2)
        fns[1].head.td_biases.data = torch.zeros(fns[1].head.td_biases.shape[0] + 1)
        with pytest.raises(ValueError, match='head 1 differs from head 0 in td_biases'):
            deploy.HeadSweep(fns, cfg, lrs=[0.1, 0.1])
        fns, cfg = _heads(2)
        fns[1].head.keep_prob = 0.9
        with pytest.raises(ValueError, match='keep_prob'):
            deploy.HeadSweep(fns, cfg, lrs=[0.1, 0.1])
        fns, cfg = _heads(2)
        with pytest.raises(ValueError, match='one learning rate per head'):
            deploy.HeadSweep(fns, cfg, lrs=[0.1])
        with pytest.raises(ValueError, match='one weight decay per head'):
            deploy.HeadSweep(fns, cfg, lrs=[0.1, 0.1], weight_decays=[0.0])
        fns, cfg = _heads(5)
        with pytest.raises(ValueError, match='1 .. 4 heads'):
            deploy.HeadSweep(fns, cfg, lrs=[0.1] * 5)
        fns, cfg = _heads(1)
        fns[0].head.softmax_att = True
        with pytest.raises(ValueError, match='spatial-softmax attention'):
            deploy.HeadSweep(fns, cfg, lrs=[0.1])
        fns, cfg = _heads(1)
        sweep = deploy.HeadSweep(fns, cfg, lrs=[0.1])
        with pytest.raises(ValueError, match='evaluate_cache'):
            sweep.best()
    finally:
        apa_config.reset_cfg()
