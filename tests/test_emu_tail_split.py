"""The producer workgroups of the one-launch tail (k_tail_fin, igmc_amd/csrc/model.hip) on the CPU emulation of the same sources.

The rows an input row of a conv layer consumes are 8 (R + 1) float4 columns, reduced in sets of 16: the row's main workgroup
takes set 0, a row producer each further set, a bias producer the layer's bias row; producers hand their sums over as tagged
words.  ``test_emu_tail_fold`` holds five relations (48 columns: three full sets).  Here:

* relation counts whose last set is partly filled or that have fewer sets -- R = 2 (24 columns: the second set half filled),
  R = 3 (32: two full sets), R = 4 (40: the third set half filled) -- four steps against the two-launch tail
  (``IGMC_TAIL_FOLD=0``): the same bits;
* the new words are waited for with the same bound: a layer whose row producers, or whose bias producer alone, publish nothing
  (emulator-only selector ``IGMC_EMU_FOLD_MUTE_ROLE``) is left untouched as a whole and reported."""
import ctypes as C

import numpy as np
import pytest

import parity_checks as PC
import test_emu_tail_fold as F
from helpers import random_rating_graph
from igmc_amd import _lib
from test_emu_tail_fold import be, data      # noqa: F401  (module-scoped fixtures: the emulator backend, the R = 5 graph)

STEPS = F.STEPS


def _data(R):
    """test_emu_tail_fold's links, on a graph of R rating levels"""
    A = random_rating_graph(44, 40, 0.3, R, seed=20)
    rows, cols = A.nonzero()
    lu, lv = rows.astype(np.int32).copy(), cols.astype(np.int32).copy()
    ly = np.asarray(A[rows, cols]).ravel().astype(np.float32)
    rng = np.random.default_rng(3)
    perm = np.concatenate([rng.permutation(len(lu)) for _ in range(2)]).astype(np.int32)
    assert len(perm) >= 7 * (STEPS + 2)
    return A, lu, lv, ly, perm


@pytest.mark.parametrize('R', [2, 3, 4])
def test_partly_filled_and_missing_sets_leave_the_bits_of_the_two_launch_tail(be, monkeypatch, R):
    monkeypatch.setattr(F, 'R', R)      # run_steps builds workspace and parameters from the module's constant
    d = _data(R)
    B, cap, cs = 7, 8, 2
    new, lab_new, ws = F.run_steps(be, d, monkeypatch, True, B, cap, cs, 0, True, 0.001, True)
    be.lib.call('igmc_model_check', ws.handle, None)      # no bounded wait ran out
    old, lab_old, _ = F.run_steps(be, d, monkeypatch, False, B, cap, cs, 0, True, 0.001, True)
    assert lab_new.get('k_tail_fin') == STEPS and 'k_tail_ts' not in lab_new and 'k_finalize_adam' not in lab_new, lab_new
    assert lab_old.get('k_tail_ts') == STEPS and lab_old.get('k_finalize_adam') == STEPS and 'k_tail_fin' not in lab_old, lab_old
    for i, (a, b) in enumerate(zip(new, old)):
        for k in a:
            assert np.array_equal(a[k], b[k]), ('step', i, k)
        assert np.isfinite(a['P']).all() and np.isfinite(a['loss']).all()
    assert not np.array_equal(new[0]['P'], new[-1]['P'])
    assert new[-1]['ctrl'][_lib.CTRL['SYNC_ERR']] == 0 and new[-1]['ctrl'][_lib.CTRL['STEP']] == 11 + STEPS


@pytest.mark.parametrize('role', ['rows', 'bias'])
def test_producer_words_that_never_arrive_leave_the_layer_untouched_and_are_reported(be, data, monkeypatch, role):
    """Conv layer 2's row producers (or its bias producer alone) publish nothing; its mains publish their own d att share.
    Every main of the layer gives up: basis, root, bias, att and their moments stay as they were, the other layers and
    lin1 / lin2 take their step, sync_err bit 8 is set and the model's check raises."""
    monkeypatch.setenv('IGMC_EMU_FOLD_MUTE_ROLE', role)
    rec, labels, ws = F.run_steps(be, data, monkeypatch, True, 7, 12, 2, 0, False, 0.001, True, steps=1, mute=2)
    assert labels.get('k_tail_fin') == 1
    lib = be.lib
    P0 = PC.flatten_params(ws, PC.make_ref_model(F.LABELS, F.R, seed=4))
    P, M1, M2 = rec[0]['P'], rec[0]['M1'], rec[0]['M2']
    cnt = C.c_int64(0)

    def span(layer, which):
        off = lib.cdll.igmc_param_offset
        off.restype, off.argtypes = C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        o = off(ws.handle, layer, which, C.byref(cnt))
        return slice(int(o), int(o) + int(cnt.value))

    for layer in range(4):
        for which in (_lib.P['BASIS'], _lib.P['ROOT'], _lib.P['BIAS'], _lib.P['ATT']):
            s = span(layer, which)
            if layer == 2:
                assert np.array_equal(P[s], P0[s]) and not M1[s].any() and not M2[s].any(), (layer, which)
            else:
                assert not np.array_equal(P[s], P0[s]) and M2[s].any(), (layer, which)
    s = span(0, _lib.P['LIN1_W'])
    assert not np.array_equal(P[s], P0[s])
    assert rec[0]['ctrl'][_lib.CTRL['SYNC_ERR']] & 8
    with pytest.raises(RuntimeError):
        lib.call('igmc_model_check', ws.handle, None)
