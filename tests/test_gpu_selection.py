"""The selection, enumeration and ranking kernels on a real MI355X, on raw keys, ids and graphs made with numpy and uploaded --
no model, no dataset, no subprocess: ``k_select_*`` (scores.hip), ``k_candidates<0/1, 0>``, ``k_segsel_part`` / ``k_segsel_merge``
(candidates.hip) and ``k_rank_check / find / count / metrics`` (ranking.hip) through their C entry points, against the numpy
references of ``tests/selection_checks.py`` -- the cases, references and checks the emulator tests run (test_emu_scores.py,
test_emu_recommend.py, test_emu_rank_eval.py).  What the single-threaded emulator cannot show is what these are for: the 64-bit
shuffle minima and float64 butterflies, ballot placement, 256 threads marking the same LDS bitmap words, 64 workgroups adding
into the same rank words, and a workgroup taking a second job where a launch is capped at 65 536 workgroups.

Every buffer sits between guard elements that are checked after every call, and the cases with inconsistent offsets, capacities
or user ids keep their bad values within the guards (an out-of-range user id is ``n_users`` or -1): a clamp the kernel lost
fails the test, it cannot leave the allocation.  Every comparison is exact but the float64 metric sums (rtol 1e-12, as in
test_emu_rank_eval.py and test_gpu_rank_eval.py)."""
import numpy as np
import pytest

import parity_checks as PC
import selection_checks as SC
from selection_checks import TILE, Guarded, P, filled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    return PC.GpuBackend()


# ------------------------------------------------------------------ extremes
@pytest.mark.parametrize('num', [1, 5, 64])
def test_select_extremes_is_the_stable_argsort(be, num):
    for n in (1, 3, 63, 64, 65, 1000, 5000, 300000):
        for name, keys in SC.key_sets(n, 100 * num + n).items():
            SC.check_extremes(be, keys, num, (0, 1, 3, 7, 1024), name)


def test_select_extremes_nan_and_signed_zero_order(be):
    SC.check_extremes_known_answer(be, (0, 1, 3, 7, 1024))


# ------------------------------------------------------------------ segmented selection
@pytest.mark.parametrize('num', [1, 5, 64])
def test_select_segments_is_the_descending_lexsort(be, num):
    SC.check_segments_layouts(be, num, (0, 1, 3, 8, 64))


def test_select_segments_one_long_segment(be):
    SC.check_segments_long(be)


def test_select_segments_nan_and_signed_zero_order(be):
    SC.check_segments_known_answer(be, (0, 1, 3, 8, 64))


def test_select_segments_of_more_segments_than_workgroups(be):
    SC.check_segments_many(be, (0, 1, 2))


# ------------------------------------------------------------------ enumeration
@pytest.mark.parametrize('n_items', [1, 63, 64, 65, 1000, TILE - 1, TILE, TILE + 1, TILE + 1000, 2 * TILE + 5])
def test_enumeration_is_the_numpy_complement(be, n_items):
    SC.check_enumeration(be, n_items)


def test_enumeration_reports_what_has_no_place_and_writes_nothing_there(be):
    SC.check_enumeration_no_place(be)


def test_enumeration_reports_what_has_no_place_on_a_graph_of_three_tiles(be):
    SC.check_enumeration_no_place(be, 40000)


def test_enumeration_reports_a_user_id_out_of_range(be):
    SC.check_enumeration_bad_user(be, (10, -1))          # n_users and -1: next to the row pointers, never far from them


def test_enumeration_of_more_users_than_workgroups(be):
    SC.check_enumeration_many_users(be)


# ------------------------------------------------------------------ ranks
@pytest.mark.parametrize('kind', SC.QUERY_KINDS)
def test_ranks_are_the_numpy_order_under_every_geometry(be, kind):
    SC.check_ranks_of_kind(be, kind, (0, 1, 3, 64))


def test_ranks_in_one_long_segment_counted_by_one_workgroup_and_by_sixty_four(be):
    SC.check_ranks_long_segment(be, (1, 64))


def test_ranks_of_more_segments_than_workgroups(be):
    SC.check_ranks_many(be, (0, 2))


def test_a_nan_scored_query_and_signed_zeros_are_ranked_by_the_word_order(be):
    SC.check_ranks_known_answer(be, (0, 1, 3, 64))


def test_ranks_agree_with_the_selection(be):
    SC.check_ranks_agree_with_the_selection(be)


@pytest.mark.parametrize('bad', SC.BAD_OFFSETS)
def test_inconsistent_offsets_are_reported_and_nothing_is_touched_out_of_range(be, bad):
    SC.check_bad_offsets(be, bad, wild=False)


# ------------------------------------------------------------------ metric sums
@pytest.mark.parametrize('ks', SC.KS_TUPLES)
def test_metric_sums_are_their_numpy_restatement_and_do_not_depend_on_the_grid(be, ks):
    SC.check_metric_sums(be, ks, (1, 3, 1000))


# ------------------------------------------------------------------ capture
def test_a_captured_select_rank_metrics_chain_replays_to_the_byte_of_the_eager_one(be):
    """``igmc_select_segments`` + ``igmc_rank_segments`` + ``igmc_rank_metrics`` recorded once (one chain, no parallel branch)
    and replayed on fresh contents of the same buffers: what ``recommend`` / ``rank_eval`` rely on when a pass replays."""
    import torch
    lib, num, geometry, ks = be.lib, 64, 3, (1, 5, 10, 1000)

    def contents(seed):
        keys, ids, off = SC.make_segments(SC.LENS, 30 + seed)
        q_off, q_id = SC.queries('mixed', keys, ids, off, seed)
        rel = (np.random.default_rng(seed).random(len(q_id)) < 0.7).astype(np.uint8)
        return keys, ids, off, q_off, q_id, rel

    keys, ids, off, q_off, q_id, rel = contents(0)
    n, ns, nq, nk = len(keys), len(off) - 1, len(q_id), len(ks)
    nbytes = lib.igmc_select_segments_scratch_bytes(ns, num, geometry)
    assert nbytes > 0 and nq > 0
    K, I = SC.guarded_keys(be, keys), Guarded(be, ids, -2 ** 31)
    O, QO, Q, R = Guarded(be, off, -1), Guarded(be, q_off, -1), Guarded(be, q_id, -2 ** 31), Guarded(be, rel, 0)
    KS, scratch = Guarded(be, np.asarray(ks, np.int32), 0), Guarded(be, np.zeros(nbytes // 8, np.int64), -3)
    err = Guarded(be, np.zeros(2, np.int32), -9)
    outs = dict(idx=(ns * num, np.int32, -9), key=(ns * num, np.float32, -9.0), cnt=(ns, np.int32, -9), pos=(nq, np.int32, -7),
                rank=(nq, np.int32, -8), mcnt=(ns * (2 + nk), np.int32, -7), mdcg=(ns * 2 * nk, np.float64, -7.0))
    out = {name: filled(be, *spec) for name, spec in outs.items()}
    err_rank, err_metrics = P(be.ptr(err.inner)), P(be.ptr(err.inner[1:]))

    def enqueue(stream):
        lib.call('igmc_select_segments', K.ptr, O.ptr, ns, num, out['idx'].ptr, out['key'].ptr, out['cnt'].ptr, scratch.ptr,
                 nbytes, geometry, stream)
        lib.call('igmc_rank_segments', K.ptr, I.ptr, n, O.ptr, ns, QO.ptr, Q.ptr, nq, out['pos'].ptr, out['rank'].ptr, err_rank,
                 geometry, stream)
        lib.call('igmc_rank_metrics', out['rank'].ptr, QO.ptr, R.ptr, nq, ns, KS.ptr, nk, out['mcnt'].ptr, out['mdcg'].ptr,
                 err_metrics, 0, stream)

    def load(case):
        for buf, values in zip((K, I, O, QO, Q, R), case):
            assert len(values) == buf.n          # (the same shapes: only the contents are fresh)
            buf.inner[:buf.n].copy_(torch.from_numpy(np.ascontiguousarray(values)))
        for name, (_, _, sentinel) in outs.items():
            out[name].inner[:out[name].n].fill_(sentinel)
        torch.cuda.synchronize()

    def results():
        torch.cuda.synchronize()
        assert err.host().tolist() == [0, 0]
        for buf in (K, I, O, QO, Q, R, KS):
            buf.check()
        scratch.host()
        return {name: out[name].host() for name in outs}

    enqueue(None)          # (first launches load code objects, which a capture cannot do)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(P(torch.cuda.current_stream().cuda_stream))
    for seed in (1, 2, 3):
        case = contents(seed)
        load(case)
        enqueue(None)
        eager = results()
        keys, ids, off, q_off, q_id, rel = case
        want = SC.expect_segments(keys, off, num)
        assert np.array_equal(eager['idx'].reshape(ns, num), want[0]) and np.array_equal(eager['cnt'], want[2])
        want_pos, want_rank = SC.rank_ref(keys, ids, off, q_off, q_id)
        assert np.array_equal(eager['pos'], want_pos) and np.array_equal(eager['rank'], want_rank)
        load(case)
        assert (out['rank'].host() == -8).all()          # (nothing of the eager run is left to be mistaken for the replay's)
        graph.replay()
        replayed = results()
        for name in outs:
            assert replayed[name].tobytes() == eager[name].tobytes(), (name, seed)
