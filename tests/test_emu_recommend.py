"""``igmc_candidates_count`` / ``igmc_candidates_fill`` and ``igmc_select_segments`` (``igmc_amd/csrc/candidates.hip``) on the CPU
emulation of the HIP sources: the enumeration is the numpy complement of every requested user's row, in (users as given,
item ascending) order, and refuses what it has no place for; the segmented selection is, per segment, THE ORDER of
``selection_checks.descending_order`` whatever the geometry.  Cases, references and checks live in ``tests/selection_checks.py``
and run unchanged on the device (``tests/test_gpu_selection.py``)."""
import numpy as np
import pytest

import selection_checks as SC
from helpers import emu_lib
from igmc_amd import engine
from parity_checks import EmuBackend
from selection_checks import TILE, graph_with_corner_rows

P = engine._p


# ------------------------------------------------------------------ enumeration
@pytest.mark.parametrize('n_items', [1, 63, 64, 65, 1000, TILE - 1, TILE, TILE + 1, TILE + 1000, 2 * TILE + 5])
def test_enumeration_is_the_numpy_complement(n_items):
    SC.check_enumeration(EmuBackend(), n_items)


def test_enumeration_reports_what_has_no_place_and_writes_nothing_there():
    SC.check_enumeration_no_place(EmuBackend())


def test_enumeration_reports_what_has_no_place_on_a_graph_of_three_tiles():
    SC.check_enumeration_no_place(EmuBackend(), 40000)


def test_enumeration_reports_a_user_id_out_of_range():
    SC.check_enumeration_bad_user(EmuBackend(), (10, -1, 2 ** 31 - 1))


@pytest.mark.slow
def test_enumeration_of_more_users_than_workgroups():
    SC.check_enumeration_many_users(EmuBackend())


def test_enumeration_refuses_bad_arguments():
    lib = emu_lib()
    g = engine.Graph(graph_with_corner_rows(4, 10, 5), lib=lib)
    users, cnt, err = np.zeros(2, np.int32), np.zeros(2, np.int64), np.zeros(1, np.int32)
    off, l = np.zeros(3, np.int64), np.zeros(64, np.int32)
    for args in ((None, P(users), 2, None, 1, P(cnt), P(err), None), (g.handle, None, 2, None, 1, P(cnt), P(err), None),
                 (g.handle, P(users), 2, None, 1, None, P(err), None), (g.handle, P(users), 2, None, 1, P(cnt), None, None),
                 (g.handle, P(users), 0, None, 1, P(cnt), P(err), None)):
        with pytest.raises(RuntimeError, match='igmc_candidates_count'):
            lib.call('igmc_candidates_count', *args)
    for args in ((g.handle, P(users), 2, None, 1, None, P(l), P(l), 64, P(err), None),
                 (g.handle, P(users), 2, None, 1, P(off), None, P(l), 64, P(err), None),
                 (g.handle, P(users), 2, None, 1, P(off), P(l), P(l), 64, None, None),
                 (g.handle, P(users), 0, None, 1, P(off), P(l), P(l), 64, P(err), None),
                 (g.handle, P(users), 2, None, 1, P(off), P(l), P(l), 0, P(err), None),
                 (g.handle, P(users), 2, None, 1, P(off), P(l), P(l), 2 ** 31, P(err), None)):
        with pytest.raises(RuntimeError, match='igmc_candidates_fill'):
            lib.call('igmc_candidates_fill', *args)


# ------------------------------------------------------------------ segmented selection
def test_the_key_set_inf_behind_nan_tells_the_two_restatements_of_the_order_apart():
    """The two-key lexsort puts a NaN in front of a -inf at a higher index; ``descending_order`` does not."""
    k = SC.key_sets(12, 0)['inf_behind_nan']
    idx = np.arange(12)
    nan, order = np.isnan(k), SC.descending_order(k, idx)
    assert nan[:2].tolist() == [True, False] and np.isneginf(k[1])
    assert not nan[order[:int((~nan).sum())]].any() and nan[order[int((~nan).sum()):]].all()
    assert order.tolist() != np.lexsort((idx, np.where(nan, np.inf, -k))).tolist()
    assert np.signbit(k[nan]).any() and not np.signbit(k[nan]).all()          # NaNs of either sign
    # all segments in one lexsort = one lexsort per segment
    keys, off = SC.key_sets(40, 1)['inf_behind_nan'], SC.offsets([0, 7, 1, 20, 0, 12])
    order, seg, place = SC.segment_places(keys, off)
    for s in range(6):
        mine = off[s] + SC.descending_order(keys[off[s]:off[s + 1]], np.arange(off[s], off[s + 1]))
        assert order[off[s]:off[s + 1]].tolist() == mine.tolist() and (seg[off[s]:off[s + 1]] == s).all()
        assert place[off[s]:off[s + 1]].tolist() == list(range(len(mine)))


@pytest.mark.parametrize('num', [1, 5, 64])
def test_select_segments_is_the_descending_lexsort(num):
    SC.check_segments_layouts(EmuBackend(), num, many_short=(0, 1, 3, 8))


def test_select_segments_one_long_segment():
    SC.check_segments_long(EmuBackend())


def test_select_segments_nan_and_signed_zero_order():
    SC.check_segments_known_answer(EmuBackend())


@pytest.mark.slow
def test_select_segments_of_more_segments_than_workgroups():
    SC.check_segments_many(EmuBackend(), (0, 2))          # (1 is what 0 chooses for this many segments: the same launch)


def test_select_segments_refuses_bad_arguments():
    lib = emu_lib()
    keys, off = np.zeros(16, np.float32), np.array([0, 16], np.int64)
    i, k, c, s = np.zeros(64, np.int32), np.zeros(64, np.float32), np.zeros(1, np.int32), np.zeros(4096, np.uint64)
    assert lib.igmc_select_segments_scratch_bytes(0, 5, 0) < 0 and lib.igmc_select_segments_scratch_bytes(1, 65, 0) < 0
    assert lib.igmc_select_segments_scratch_bytes(1, 0, 0) < 0 and lib.igmc_select_segments_scratch_bytes(1, 5, 65) < 0
    assert lib.igmc_select_segments_scratch_bytes(1, 5, -1) < 0
    assert lib.igmc_select_segments_scratch_bytes(7, 5, 3) == 7 * 3 * 5 * 8
    for ns, num, nbytes, geometry in ((0, 5, 32768, 0), (1, 0, 32768, 0), (1, 65, 32768, 0), (1, 5, 8, 3), (1, 5, 32768, -1),
                                      (1, 5, 32768, 65)):
        with pytest.raises(RuntimeError, match='igmc_select_segments'):
            lib.call('igmc_select_segments', P(keys), P(off), ns, num, P(i), P(k), P(c), P(s), nbytes, geometry, None)
    for args in ((None, P(off), 1, 5, P(i), P(k), P(c), P(s), 32768, 0, None),
                 (P(keys), None, 1, 5, P(i), P(k), P(c), P(s), 32768, 0, None),
                 (P(keys), P(off), 1, 5, None, P(k), P(c), P(s), 32768, 0, None),
                 (P(keys), P(off), 1, 5, P(i), P(k), None, P(s), 32768, 0, None),
                 (P(keys), P(off), 1, 5, P(i), P(k), P(c), None, 32768, 0, None)):
        with pytest.raises(RuntimeError, match='igmc_select_segments: null'):
            lib.call('igmc_select_segments', *args)
    lib.call('igmc_select_segments', P(keys), P(off), 1, 5, P(i), None, P(c), P(s), 32768, 0, None)      # keys out: optional
