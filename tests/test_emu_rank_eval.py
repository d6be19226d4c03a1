"""``igmc_rank_segments`` / ``igmc_rank_metrics`` (``igmc_amd/csrc/ranking.hip``) on the CPU emulation of the HIP sources: the rank
of a queried id is its place in THE ORDER (``selection_checks.descending_order``) of its segment whatever the geometry
(and the place ``igmc_select_segments`` gives it), ids a segment does not hold come back as -1 / -1, the metric sums are their
numpy float64 restatement and do not depend on the grid, and inconsistent query offsets are reported, not followed.  Cases,
references and checks live in ``tests/selection_checks.py`` and run unchanged on the device (``tests/test_gpu_selection.py``)."""
import numpy as np
import pytest

import selection_checks as SC
from helpers import emu_lib
from igmc_amd import engine
from parity_checks import EmuBackend

P = engine._p


@pytest.mark.parametrize('kind', SC.QUERY_KINDS)
def test_ranks_are_the_numpy_order_under_every_geometry(kind):
    SC.check_ranks_of_kind(EmuBackend(), kind)


def test_the_reference_without_a_loop_is_the_reference():
    keys, ids, off = SC.make_segments(SC.LENS, 11)
    for kind in SC.QUERY_KINDS[1:]:
        q_off, q_id = SC.queries(kind, keys, ids, off, 5)
        for a, b in zip(SC.rank_ref(keys, ids, off, q_off, q_id), SC.rank_ref_flat(keys, ids, off, q_off, q_id)):
            assert np.array_equal(a, b), kind


def test_a_nan_scored_query_and_signed_zeros_are_ranked_by_the_word_order():
    SC.check_ranks_known_answer(EmuBackend())


def test_ranks_agree_with_the_selection():
    SC.check_ranks_agree_with_the_selection(EmuBackend())


def test_ranks_in_one_long_segment_counted_by_one_workgroup_and_by_sixty_four():
    SC.check_ranks_long_segment(EmuBackend())


@pytest.mark.slow
def test_ranks_of_more_segments_than_workgroups():
    SC.check_ranks_many(EmuBackend())


# ------------------------------------------------------------------ metrics
@pytest.mark.parametrize('ks', SC.KS_TUPLES)
def test_metric_sums_are_their_numpy_restatement_and_do_not_depend_on_the_grid(ks):
    SC.check_metric_sums(EmuBackend(), ks)


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize('bad', SC.BAD_OFFSETS)
def test_inconsistent_query_offsets_are_reported_and_nothing_is_touched_out_of_range(bad):
    SC.check_bad_offsets(EmuBackend(), bad, wild=True)


def test_rank_entry_points_refuse_bad_arguments():
    lib = emu_lib()
    keys, ids = np.zeros(16, np.float32), np.arange(16, dtype=np.int32)
    off, q_off, q = np.array([0, 16], np.int64), np.array([0, 2], np.int64), np.array([3, 4], np.int32)
    pos, rank, err = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(1, np.int32)
    good = [P(keys), P(ids), 16, P(off), 1, P(q_off), P(q), 2, P(pos), P(rank), P(err), 0, None]
    lib.call('igmc_rank_segments', *good)
    assert err[0] == 0 and pos.tolist() == [3, 4]
    for i, v in ((0, None), (1, None), (3, None), (5, None), (6, None), (8, None), (9, None), (10, None), (2, 0), (2, 2 ** 31),
                 (4, 0), (7, -1), (11, -1), (11, 65)):
        args = list(good)
        args[i] = v
        with pytest.raises(RuntimeError, match='igmc_rank_segments'):
            lib.call('igmc_rank_segments', *args)
    ks, cnt, dcg = np.array([5], np.int32), np.zeros(3, np.int32), np.zeros(2, np.float64)
    good = [P(rank), P(q_off), None, 2, 1, P(ks), 1, P(cnt), P(dcg), P(err), 0, None]
    lib.call('igmc_rank_metrics', *good)
    for i, v in ((0, None), (1, None), (5, None), (7, None), (8, None), (9, None), (3, -1), (4, 0), (6, 0), (6, 9), (10, -1)):
        args = list(good)
        args[i] = v
        with pytest.raises(RuntimeError, match='igmc_rank_metrics'):
            lib.call('igmc_rank_metrics', *args)
