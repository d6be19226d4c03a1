"""``igmc_scores_store`` and ``igmc_select_extremes`` (``igmc_amd/csrc/scores.hip``) on the CPU emulation of the HIP sources:
the scoring step's tail files outputs and labels at their positions of the pass, sums exactly as ``igmc_sse_accumulate`` and
reports a position it has no place for; the selection of the extremes is ``np.argsort(kind='stable')`` whatever the grid."""
import ctypes as C

import numpy as np
import pytest

import selection_checks as SC
from helpers import emu_lib, load_extract_golden
from igmc_amd import _lib, engine
from igmc_amd.stepgraph import _ctrl_words
from parity_checks import EmuBackend

CASES = load_extract_golden()
P = engine._p


def _setup(lib, B=4):
    case = CASES['synth_cap']
    g = engine.Graph(case['A'], lib=lib)
    lu = case['links'][:, 0].astype(np.int32).copy()
    lv = case['links'][:, 1].astype(np.int32).copy()
    ly = case['class_values'][case['link_labels']].astype(np.float32)
    return case, g, lu, lv, ly


def _store(lib, out, batch, acc, scores, labels, first, err, ctrl=None):
    lib.call('igmc_scores_store', P(out), batch.handle, P(acc), P(scores), P(labels), len(scores), int(first),
             P(ctrl), P(err), None)


def test_scores_land_at_their_positions_and_the_sums_are_sse_accumulates():
    lib = emu_lib()
    case, g, lu, lv, ly = _setup(lib)
    n, B = len(lu), 4
    assert n >= 3 * B
    perm = np.random.default_rng(1).permutation(n).astype(np.int32)
    batch = engine.Batch(g, B, 1, case['mnph'])
    rng = np.random.default_rng(2)
    scores, labels = np.full(n, -77.0, np.float32), np.full(n, -88.0, np.float32)
    acc, acc_ref, err = np.zeros(2, np.float64), np.zeros(2, np.float64), np.zeros(1, np.int32)
    want_s, want_y = scores.copy(), labels.copy()
    # batches 0 and 2 of the pass, and a ragged one at the end: batch 1's positions stay untouched
    for first, nb in ((0, B), (2 * B, B), (n - 3, 3)):
        batch.extract(lu, lv, ly, perm, first, nb, 1.0, 7, 0)
        out = rng.normal(3.0, 1.0, B).astype(np.float32)
        _store(lib, out, batch, acc, scores, labels, first, err)
        lib.call('igmc_sse_accumulate', P(out), batch.handle, P(acc_ref), None)
        want_s[first:first + nb] = out[:nb]
        want_y[first:first + nb] = ly[perm[first:first + nb]]
        assert np.array_equal(scores, want_s) and np.array_equal(labels, want_y)
    assert err[0] == 0
    assert np.array_equal(scores[B:2 * B], np.full(B, -77.0, np.float32))
    assert acc.tobytes() == acc_ref.tobytes() and acc[1] == 2 * B + 3


def test_position_comes_from_the_arenas_stamp_under_the_step_control_and_the_tick_is_the_evaluation_steps():
    lib = emu_lib()
    case, g, lu, lv, ly = _setup(lib)
    n, B, M = len(lu), 4, 2
    perm = np.arange(n, dtype=np.int32)
    ctrl = _ctrl_words(1, 0, 1, B, M, 0.0, 0.9, 0.999, 1e-8, 0.0)
    ctrl_ref = ctrl.copy()
    arenas = [engine.Batch(g, B, 1, case['mnph']) for _ in range(M)]
    for a in arenas:
        lib.call('igmc_batch_set_ctrl', a.handle, C.c_void_p(ctrl.ctypes.data))
    scores, labels = np.full(n, -1.0, np.float32), np.full(n, -1.0, np.float32)
    acc, acc_ref, err = np.zeros(2, np.float64), np.zeros(2, np.float64), np.zeros(1, np.int32)
    outs = np.random.default_rng(3).normal(3.0, 1.0, (M, B)).astype(np.float32)
    for i, a in enumerate(arenas):          # batch i of the group of parity 0: selector 0 | (i << 1)
        a.extract(lu, lv, ly, perm, i << 1, B, 1.0, 7, 0)
    for i, a in enumerate(arenas):
        _store(lib, outs[i], a, acc, scores, labels, -1, err, ctrl)
        lib.call('igmc_sse_accumulate_tick', P(outs[i]), a.handle, P(acc_ref), P(ctrl_ref), None)
    assert err[0] == 0
    assert np.array_equal(scores[:M * B], outs.reshape(-1)) and np.array_equal(labels[:M * B], ly[:M * B])
    assert np.array_equal(scores[M * B:], np.full(n - M * B, -1.0, np.float32))
    assert acc.tobytes() == acc_ref.tobytes()
    assert np.array_equal(ctrl, ctrl_ref)          # the same tick: cursors, counters, parity


def test_a_position_without_a_place_is_reported_and_writes_nothing():
    lib = emu_lib()
    case, g, lu, lv, ly = _setup(lib)
    n, B = len(lu), 4
    batch = engine.Batch(g, B, 1, case['mnph'])
    batch.extract(lu, lv, ly, None, 0, B, 1.0, 7, 0)
    out = np.arange(B, dtype=np.float32)
    guard = 8
    for cap, first, bit, written in ((6, 4, 1, 2), (6, -1, 2, 0)):
        # (cap 6, first 4: positions 4, 5 exist, 6, 7 do not; first -1 on an arena without a control block: no stamp)
        scores, labels = np.full(cap + guard, -5.0, np.float32), np.full(cap + guard, -6.0, np.float32)
        acc, err = np.zeros(2, np.float64), np.zeros(1, np.int32)
        lib.call('igmc_scores_store', P(out), batch.handle, P(acc), P(scores), P(labels), cap, first, None, P(err), None)
        assert err[0] == bit
        assert np.array_equal(scores[cap:], np.full(guard, -5.0, np.float32))          # nothing past the capacity
        assert np.array_equal(labels[cap:], np.full(guard, -6.0, np.float32))
        assert int((scores[:cap] != -5.0).sum()) == written
        assert acc[1] == B          # the sums are the evaluation step's in every case
    # bad arguments fail through the C ABI's error path
    acc, err = np.zeros(2, np.float64), np.zeros(1, np.int32)
    s = np.zeros(8, np.float32)
    for args in ((0, 0), (8, 8), (8, -2)):
        with pytest.raises(RuntimeError, match='igmc_scores_store'):
            lib.call('igmc_scores_store', P(out), batch.handle, P(acc), P(s), P(s), args[0], args[1], None, P(err), None)
    with pytest.raises(RuntimeError, match='null'):
        lib.call('igmc_scores_store', P(out), batch.handle, P(acc), P(s), P(s), 8, 0, None, None, None)


# ------------------------------------------------------------------ selection of the extremes
# (cases, reference and checks: tests/selection_checks.py, shared with tests/test_gpu_selection.py)
@pytest.mark.parametrize('num', [1, 5, 64])
def test_select_extremes_is_the_stable_argsort(num):
    be = EmuBackend()
    sizes = sorted(set(s for s in (1, 3, num - 1, num, num + 1, 64, 65, 1000, 5000) if s >= 1))
    for n in sizes:
        for name, keys in SC.key_sets(n, 100 * num + n).items():
            SC.check_extremes(be, keys, num, (0, 1, 3, 7), name)


def test_select_extremes_nan_and_signed_zero_order():
    SC.check_extremes_known_answer(EmuBackend())


def test_select_extremes_refuses_bad_arguments():
    lib = emu_lib()
    keys = np.zeros(16, np.float32)
    i, k, s = np.zeros(64, np.int32), np.zeros(64, np.float32), np.zeros(4096, np.uint64)
    assert lib.igmc_select_scratch_bytes(0, 5, 0) < 0 and lib.igmc_select_scratch_bytes(16, 65, 0) < 0
    assert lib.igmc_select_scratch_bytes(16, 5, 2000) < 0 and lib.igmc_select_scratch_bytes(2 ** 31, 5, 0) < 0
    assert lib.igmc_select_scratch_bytes(16, 5, 3) == 2 * 3 * 5 * 8
    for n, num, nbytes, grid in ((0, 5, 4096, 0), (16, 0, 4096, 0), (16, 65, 32768, 0), (16, 5, 8, 0), (16, 5, 4096, -1)):
        with pytest.raises(RuntimeError, match='igmc_select_extremes'):
            lib.call('igmc_select_extremes', P(keys), n, num, P(i), P(i), P(k), P(k), None, P(s), nbytes, grid, None)
    with pytest.raises(RuntimeError, match='null'):
        lib.call('igmc_select_extremes', None, 16, 5, P(i), P(i), P(k), P(k), None, P(s), 4096, 0, None)
