"""The one-launch tail (k_tail_fin: mains, row producers, bias producers) against the two-launch tail on the device at the
smallest slot counts of the partial tables: ml_1m, cap 100, edge dropout 0.2, steps launched eagerly.

* B = 1: 4 table slots (one cluster of four) -- fewer than the 16 partial groups of the reduction, so most groups sum nothing
  and every load past the fourth slot is a clamped one (``ts_slot``);
* B = 17: 68 slots -- no multiple of 16, so the groups hold 5 and 4 slots.

(``test_gpu_tail_fold`` holds 28 and 200 slots.)  Parameters, both Adam moments, the flat gradient, the loss words, the epoch
total, the control block and the weight images must be the same bits, and no bounded wait may run out."""
import gc

import pytest

import test_gpu_tail_fold as F

pytestmark = pytest.mark.gpu

ml1m = F.ml1m      # (module-scoped fixture: the ml_1m case of test_gpu_headline)


@pytest.mark.parametrize('B', [1, 17])
def test_few_table_slots_leave_the_bits_of_the_two_launch_tail(ml1m, monkeypatch, B):
    import torch
    import test_gpu_headline as H
    from igmc_amd.util_functions import MyDynamicDataset
    A, links, labels, cv = ml1m['A'], ml1m['links'], ml1m['link_labels'], ml1m['class_values']
    ds = MyDynamicDataset('data/t/split', A, (links[:, 0], links[:, 1]), labels, 1, 1.0, 100, None, None, cv, device=0, seed=1)
    perm = torch.randperm(len(ds), generator=torch.Generator().manual_seed(5))
    new_e, lab_new = F._run(ds, B, 0.2, perm, True, monkeypatch, use_graph=False, overlap=False)      # (_run: sg.check() is clean)
    old_e, lab_old = F._run(ds, B, 0.2, perm, False, monkeypatch, use_graph=False, overlap=False)
    assert lab_new.get('k_tail_fin') == F.STEPS and 'k_tail_ts' not in lab_new and 'k_finalize_adam' not in lab_new, lab_new
    assert lab_old.get('k_tail_ts') == F.STEPS and lab_old.get('k_finalize_adam') == F.STEPS and 'k_tail_fin' not in lab_old, lab_old
    assert new_e[8] == F.STEPS and torch.isfinite(new_e[0]).all()
    H._assert_same(new_e, old_e, 'eager steps, one-launch tail vs two-launch tail, B = %d' % B)
    gc.collect()      # (the four step objects and their device memory go here, not at a moment of a later test's choosing)
