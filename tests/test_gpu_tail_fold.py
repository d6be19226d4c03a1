"""The tail of the subgraph kernel as ONE launch (k_tail_fin) against the two-launch tail (k_tail_ts -> k_finalize_ts,
``IGMC_TAIL_FOLD=0``) on the device, at the headline shape: ml_1m, cap 100, batches of 50 (200 partial tables: clusters of
four) and of 7, with and without edge dropout.  Five steps launched eagerly, and nine with eight of them replayed as a pair of
hipGraph groups of four, must leave the same bits either way: parameters, both Adam moments, the flat gradient, the loss
words, the epoch total, the control block and the weight images the last step left for the next one; no bounded wait may
run out (``StepGraph.check``)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 5


@pytest.fixture(scope='module')
def ml1m():
    import test_gpu_headline as H
    return H.ml_case('ml_1m', 100, 600)


def _images(sg):
    import torch
    fn = sg.lib.cdll.igmc_debug_weight_images
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    n = C.c_int64(0)
    assert fn(sg.ws.handle, None, C.byref(n)) == 0 and n.value > 0
    out = np.zeros(n.value, np.uint32)
    torch.cuda.synchronize()
    assert fn(sg.ws.handle, C.c_void_p(out.ctypes.data), C.byref(n)) == 0
    return torch.from_numpy(out.view(np.int32).copy())


def _run(ds, B, drop, perm, fold, monkeypatch, **sg_kw):
    """STEPS eager steps of StepGraph from one seed -- or, with graphs, one eager step and a replayed pair of groups; what they
    leave behind, and (eager) the kernels that ran."""
    import torch
    from igmc_amd import engine
    from igmc_amd.models import IGMC
    from igmc_amd.stepgraph import StepGraph
    from igmc_amd.train_eval import FlatAdam
    if fold:
        monkeypatch.delenv('IGMC_TAIL_FOLD', raising=False)
    else:
        monkeypatch.setenv('IGMC_TAIL_FOLD', '0')
    torch.manual_seed(3)
    model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True, adj_dropout=drop,
                 seed=1).to('cuda')
    model.reset_parameters()
    opt = FlatAdam(model, lr=1e-3)
    sg = StepGraph(model, opt, ds, B, 0.001, **sg_kw)
    assert sg.ws.dense_path(sg.arenas[0], B)
    sg.begin_epoch(perm, 1)
    eager = not sg_kw.get('use_graph', True)
    if eager:
        engine.profile_fetch(sg.lib)
        engine.profile_enable(sg.lib, True)
    try:
        if eager:
            sg.steps(STEPS)
        else:
            sg.steps(1)
            sg.steps(2 * sg.M)
            assert any(g is not None for g in sg.graphs)
        torch.cuda.synchronize()
    finally:
        if eager:
            engine.profile_enable(sg.lib, False)
    labels = {n: c for n, _, c in engine.profile_fetch(sg.lib)} if eager else None
    sg.check()                                   # raises if a bounded device-side wait timed out
    torch.cuda.synchronize()
    res = (model.flat_parameters().detach().cpu().clone(), opt.exp_avg.detach().cpu().clone(),
           opt.exp_avg_sq.detach().cpu().clone(), model.flat_grad().detach().cpu().clone(), sg.loss.cpu().clone(),
           sg.total.cpu().clone(), sg.ctrl.cpu().clone(), _images(sg), opt.t)
    return res, labels


@pytest.mark.parametrize('drop', [0.0, 0.2])
@pytest.mark.parametrize('B', [50, 7])
def test_one_launch_tail_leaves_the_bits_of_the_two_launch_tail(ml1m, monkeypatch, B, drop):
    import torch
    import test_gpu_headline as H
    from igmc_amd.util_functions import MyDynamicDataset
    A, links, labels, cv = ml1m['A'], ml1m['links'], ml1m['link_labels'], ml1m['class_values']
    ds = MyDynamicDataset('data/t/fold', A, (links[:, 0], links[:, 1]), labels, 1, 1.0, 100, None, None, cv, device=0, seed=1)
    perm = torch.randperm(len(ds), generator=torch.Generator().manual_seed(5))
    new_e, lab_new = _run(ds, B, drop, perm, True, monkeypatch, use_graph=False, overlap=False)
    old_e, lab_old = _run(ds, B, drop, perm, False, monkeypatch, use_graph=False, overlap=False)
    # the launches of a step: the subgraph kernel and ONE tail launch -- two with the switch off
    assert lab_new.get('k_tail_fin') == STEPS and 'k_tail_ts' not in lab_new and 'k_finalize_adam' not in lab_new, lab_new
    assert lab_old.get('k_tail_ts') == STEPS and lab_old.get('k_finalize_adam') == STEPS and 'k_tail_fin' not in lab_old, lab_old
    assert new_e[8] == STEPS and torch.isfinite(new_e[0]).all()
    H._assert_same(new_e, old_e, 'eager steps, one-launch tail vs two-launch tail')
    new_g, _ = _run(ds, B, drop, perm, True, monkeypatch, group=4)
    old_g, _ = _run(ds, B, drop, perm, False, monkeypatch, group=4)
    assert new_g[8] == 1 + 2 * 4
    H._assert_same(new_g, old_g, 'groups of 4, one-launch tail vs two-launch tail')
