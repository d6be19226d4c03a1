"""Conv layer 3's weight gradient as centre vectors (``StepPlan::l3_vec``) against the per-workgroup tables it replaces
(``IGMC_L3_VEC=0``) on the device: ml_1m, cap 100, clusters of four.

* B = 9 (36 slots at stride 16: slot ids with holes, two or three slots a partial group) and B = 50 (the headline's 200 slots),
  dropout 0 and 0.2, both tails (``k_tail_fin``, and ``k_tail_ts`` -> ``k_finalize_ts`` under ``IGMC_TAIL_FOLD=0``): three steps
  launched eagerly must leave the same bits either way -- parameters, both Adam moments, the flat gradient, the loss words, the
  epoch total, the control block and the weight images -- and no bounded wait may run out;
* one eager step and two replayed hipGraph groups of four leave what nine eager steps leave, and what the tables leave.

(``test_emu_l3_vectors`` holds the small shapes on the CPU emulation of the same sources.)"""
import gc

import pytest

import test_gpu_tail_fold as F

pytestmark = pytest.mark.gpu

ml1m = F.ml1m      # (module-scoped fixture: the ml_1m case of test_gpu_headline)


def _ds(ml1m):
    from igmc_amd.util_functions import MyDynamicDataset
    A, links, labels, cv = ml1m['A'], ml1m['links'], ml1m['link_labels'], ml1m['class_values']
    return MyDynamicDataset('data/t/l3vec', A, (links[:, 0], links[:, 1]), labels, 1, 1.0, 100, None, None, cv, device=0, seed=1)


def _run(ds, B, drop, perm, vec, fold, monkeypatch, steps, **sg_kw):
    """test_gpu_tail_fold._run under IGMC_L3_VEC unset / 0, with `steps` eager steps"""
    if vec:
        monkeypatch.delenv('IGMC_L3_VEC', raising=False)
    else:
        monkeypatch.setenv('IGMC_L3_VEC', '0')
    monkeypatch.setattr(F, 'STEPS', steps)
    return F._run(ds, B, drop, perm, fold, monkeypatch, **sg_kw)


def _planned(ds, B, monkeypatch, vec):
    """igmc_debug_l3_vectors of a step on the dataset's arena under the hook"""
    from igmc_amd.models import IGMC
    from igmc_amd.stepgraph import StepGraph
    from igmc_amd.train_eval import FlatAdam
    if vec:
        monkeypatch.delenv('IGMC_L3_VEC', raising=False)
    else:
        monkeypatch.setenv('IGMC_L3_VEC', '0')
    model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True, adj_dropout=0.0, seed=1).to('cuda')
    sg = StepGraph(model, FlatAdam(model, lr=1e-3), ds, B, 0.001, use_graph=False, overlap=False)
    return sg.ws.l3_vectors(sg.arenas[0], B)


@pytest.mark.parametrize('fold', [True, False], ids=['k_tail_fin', 'k_tail_ts'])
@pytest.mark.parametrize('drop', [0.0, 0.2])
@pytest.mark.parametrize('B', [9, 50])
def test_centre_vectors_leave_the_bits_of_the_tables(ml1m, monkeypatch, B, drop, fold):
    import torch
    import test_gpu_headline as H
    ds = _ds(ml1m)
    perm = torch.randperm(len(ds), generator=torch.Generator().manual_seed(5))
    assert _planned(ds, B, monkeypatch, True) == 2 and _planned(ds, B, monkeypatch, False) == 0      # clusters of four: member 2
    new, lab_new = _run(ds, B, drop, perm, True, fold, monkeypatch, 3, use_graph=False, overlap=False)      # (_run: sg.check() is clean)
    old, lab_old = _run(ds, B, drop, perm, False, fold, monkeypatch, 3, use_graph=False, overlap=False)
    tail = 'k_tail_fin' if fold else 'k_tail_ts'
    assert lab_new.get(tail) == 3 and lab_old.get(tail) == 3 and lab_new.get('k_graph_step') == 3, (lab_new, lab_old)
    assert new[8] == 3 and torch.isfinite(new[0]).all()
    H._assert_same(new, old, 'three eager steps, centre vectors vs tables, B = %d' % B)
    gc.collect()      # (the step objects and their device memory go here, not at a moment of a later test's choosing)


def test_replayed_groups_equal_the_eager_steps(ml1m, monkeypatch):
    import test_gpu_headline as H
    import torch
    ds = _ds(ml1m)
    perm = torch.randperm(len(ds), generator=torch.Generator().manual_seed(5))
    new_g, _ = _run(ds, 50, 0.2, perm, True, True, monkeypatch, 9, group=4)
    old_g, _ = _run(ds, 50, 0.2, perm, False, True, monkeypatch, 9, group=4)
    new_e, _ = _run(ds, 50, 0.2, perm, True, True, monkeypatch, 9, use_graph=False, overlap=False)
    assert new_g[8] == 9 and new_e[8] == 9
    H._assert_same(new_g, old_g, 'groups of 4, centre vectors vs tables')
    # (what a step leaves for the next one, whatever launched it: parameters, moments, gradient, weight images, Adam's count)
    H._assert_same(new_g[:4] + new_g[7:], new_e[:4] + new_e[7:], 'centre vectors: groups of 4 vs nine eager steps')
    gc.collect()
