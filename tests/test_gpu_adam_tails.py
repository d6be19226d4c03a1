"""Every Adam tail against float64 Adam, element by element, on the device (tests/adam_checks.py; CPU twin:
tests/test_emu_adam_tails.py): the same rows, shapes, hyper-parameters and Adam steps through the gfx950 library -- and the
learning-rate schedule of ``train_multiple_epochs`` through the replayed step graph, whose captured launches carry the old
learning rate as an argument and must take the new one from the control block."""
import numpy as np
import pytest

import adam_checks as AC
import parity_checks as PC
from adam_checks import H0, H1

pytestmark = pytest.mark.gpu

CASES, IDS = AC.CASES, AC.IDS


@pytest.fixture(scope='module')
def be():
    return PC.GpuBackend()


@pytest.mark.parametrize('row,B,drop,hyp,ts,t_ctrl', CASES, ids=IDS)
def test_scalars_as_arguments(be, monkeypatch, row, B, drop, hyp, ts, t_ctrl):
    for t in ts:
        AC.check_step(be, monkeypatch, row, B, drop, hyp, t, 'args')


@pytest.mark.parametrize('row,B,drop,hyp,ts,t_ctrl', CASES, ids=IDS)
def test_scalars_from_the_control_block_three_steps_and_a_new_learning_rate(be, monkeypatch, row, B, drop, hyp, ts, t_ctrl):
    AC.check_step(be, monkeypatch, row, B, drop, hyp, t_ctrl, 'ctrl')


@pytest.mark.parametrize('n', [1, 2047, 2049, 49233])
@pytest.mark.parametrize('hyp', [H0, H1], ids=['H0', 'H1'])
def test_flat_adam(be, n, hyp):
    for t in AC.T_STEPS:
        AC.check_flat_adam(be, n, hyp, t)
    AC.check_flat_adam(be, n, hyp, 7, route='ctrl')


@pytest.mark.parametrize('row,B,drop', [('fold_cs1', 7, True), ('fold_cs4', 17, False), ('ts_cs2', 7, True), ('dense_r5', 7, True)])
def test_weight_images_left_by_a_weight_decayed_step_equal_the_composed_ones(be, monkeypatch, row, B, drop):
    AC.check_images(be, monkeypatch, row, B, drop)


# ====================================================================== the schedule through the step graph
def _schedule_run(ds, perm, decay, **sg_kw):
    """Two epochs of StepGraph from Adam step 1000 and non-zero moments (loaded through ``load_state_dict``), H1; after the
    first epoch the learning rate is multiplied by ``decay`` the way ``train_multiple_epochs`` does."""
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.stepgraph import StepGraph
    from igmc_amd.train_eval import FlatAdam
    torch.manual_seed(3)
    model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True, adj_dropout=0.2, seed=1).to('cuda')
    model.reset_parameters()
    lr, b1, b2, eps, wd = H1
    opt = FlatAdam(model, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    m1, m2 = AC.start_moments(model.flat_parameters().numel())
    where = {k: (o, n, s) for (k, o, n, s) in model._views}
    state = {}
    for i, (k, _) in enumerate(model.named_parameters()):
        o, n, s = where[k]
        state[i] = dict(step=torch.tensor(1000.0), exp_avg=torch.from_numpy(m1[o:o + n].copy()).view(s),
                        exp_avg_sq=torch.from_numpy(m2[o:o + n].copy()).view(s))
    opt.load_state_dict(dict(state=state, param_groups=[dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)]))
    assert opt.t == 1000 and np.array_equal(opt.exp_avg_sq.cpu().numpy(), m2)
    sg = StepGraph(model, opt, ds, 50, 0.001, **sg_kw)
    totals = []
    for ep in (1, 2):
        t, n = sg.run_epoch(perm, ep)
        totals.append(float(t.item()))
        if ep == 1:
            opt.param_groups[0]['lr'] *= decay          # (reference train_eval.py:94-96)
    torch.cuda.synchronize()
    return sg, opt, (model.flat_parameters().detach().cpu().clone(), opt.exp_avg.detach().cpu().clone(),
                     opt.exp_avg_sq.detach().cpu().clone(), totals, opt.t)


def test_a_decayed_learning_rate_reaches_the_replayed_step_graph():
    import torch
    import test_gpu_headline as H
    from igmc_amd import _lib
    from igmc_amd.util_functions import MyDynamicDataset
    case = H.ml_case('ml_1m', 100, 250)
    A, cv = case['A'], case['class_values']
    coo = A.tocoo()
    pick = np.random.default_rng(11).permutation(coo.nnz)[:1200]
    u, v, y = coo.row[pick], coo.col[pick], (coo.data[pick] - 1).astype(np.int64)
    ds = MyDynamicDataset('data/t/adam_schedule', A, (u, v), y, 1, 1.0, 100, None, None, cv, device=0, seed=1)
    perm = torch.randperm(len(ds), generator=torch.Generator().manual_seed(5))
    sg, opt, ref = _schedule_run(ds, perm, 0.1, group=8)
    assert any(g is not None for g in sg.graphs) and ref[4] == 1000 + 48
    assert all(torch.isfinite(x).all() for x in ref[:3])
    # the control block after epoch 2: the decayed learning rate, and a step size that belongs to its own step counter
    w = sg.ctrl.cpu().numpy()
    d = AC.ctrl_doubles(w)
    lr2 = H1[0] * 0.1
    assert opt.param_groups[0]['lr'] == lr2 and d[_lib.CTRL['LR']] == lr2
    assert int(w[_lib.CTRL['ADAM_T']]) == opt.t + 1
    AC.check_ctrl_advanced(w, opt.t + 1, (lr2, d[_lib.CTRL['BETA1']], d[_lib.CTRL['BETA2']]), 'after epoch 2')
    assert d[_lib.CTRL['BETA1']] == H1[1] and d[_lib.CTRL['BETA2']] == H1[2] and d[_lib.CTRL['EPS']] == H1[3]
    assert d[_lib.CTRL['WD']] == H1[4]
    sg_e, _, eager = _schedule_run(ds, perm, 0.1, use_graph=False, overlap=False, group=8)
    assert not any(g is not None for g in sg_e.graphs)
    H._assert_same(ref, eager, 'replayed groups of 8 vs eager one-stream launches, learning rate decayed after epoch 1')
    _, _, flat = _schedule_run(ds, perm, 1.0, group=8)
    assert flat[4] == ref[4] and not torch.equal(flat[0], ref[0]), 'the decayed learning rate changed nothing'
    # (the moments see the decay through the parameters the second epoch's gradients are taken at)
    assert not torch.equal(flat[1], ref[1])
