"""The tail of the subgraph kernel as ONE launch (k_tail_fin, igmc_amd/csrc/model.hip) against the two-launch tail it replaces
(k_tail_ts -> k_finalize_ts, ``IGMC_TAIL_FOLD=0``), on the CPU emulation of the same sources, which runs the workgroups of a
layer together.  Every sum keeps its order, so four consecutive ``igmc_train_step`` calls from the same state must leave the
SAME BITS: parameters, both Adam moments, the flat gradient, the loss words, the epoch total, the control block and the weight
images the step leaves for the next one.

Shapes: five relations, one hop (four labels), per-hop caps of 8..16 -- and batch sizes / cluster sizes that give every slot
count the reduction distinguishes: fewer slots than partial groups (< 16), a count that is no multiple of 16, and 200 (the
headline's: 50 subgraphs x 4 members); one workgroup per subgraph, clusters of 2 and 4, the looping grid (fewer workgroups
than subgraphs); with and without edge dropout; ARR 0 and 0.001; Adam scalars from the control block and from the arguments.

(The emulator runs every work-item of the subgraph kernel as a fiber: the case of 50 subgraphs takes it about two minutes, the
others seconds.)

The hand-off is bounded: a layer whose words never arrive (emulator-only switch) is left untouched and reported."""
import ctypes as C
import struct

import numpy as np
import pytest

import parity_checks as PC
from helpers import random_rating_graph
from igmc_amd import _lib, engine

R, LABELS, STEPS = 5, 4, 4


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


@pytest.fixture(scope='module')
def data():
    A = random_rating_graph(44, 40, 0.3, R, seed=20)
    rows, cols = A.nonzero()
    lu, lv = rows.astype(np.int32).copy(), cols.astype(np.int32).copy()
    ly = np.asarray(A[rows, cols]).ravel().astype(np.float32)
    rng = np.random.default_rng(3)
    perm = np.concatenate([rng.permutation(len(lu)) for _ in range(2)]).astype(np.int32)
    assert len(perm) >= 50 * (STEPS + 2)
    return A, lu, lv, ly, perm


def _ctrl_words(B):
    """Control block that describes step 11 (Adam step 1) of batches of B: the step's last kernel advances it."""
    w = np.zeros(_lib.CTRL['WORDS'], np.int64)
    w[0], w[1], w[2], w[3], w[4] = 11, 0, 3, 1, B
    w[6], w[7] = B, 0
    for k, v in ((8, 1e-3), (9, 0.9), (10, 0.999), (11, 1e-8), (12, 0.0), (13, 1e-3 / (1 - 0.9)), (14, 1.0 / (1 - 0.999) ** 0.5)):
        w[k] = struct.unpack('<q', struct.pack('<d', float(v)))[0]
    return w


def _images(lib, ws):
    fn = lib.cdll.igmc_debug_weight_images
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    n = C.c_int64(0)
    assert fn(ws.handle, None, C.byref(n)) == 0 and n.value > 0
    out = np.zeros(n.value, np.uint32)
    assert fn(ws.handle, C.c_void_p(out.ctypes.data), C.byref(n)) == 0
    return out


def run_steps(be, data, monkeypatch, fold, B, cap, cs, grid, drop, ARR, use_ctrl, steps=STEPS, mute=None):
    """`steps` fused steps on consecutive batches from one initial state; everything a step leaves, per step."""
    lib = be.lib
    A, lu, lv, ly, perm = data
    monkeypatch.setenv('IGMC_GRAPH_STEP', '1')
    monkeypatch.setenv('IGMC_GS_CLUSTER', str(cs))
    monkeypatch.setenv('IGMC_TAIL_FOLD', '1' if fold else '0')
    if grid:
        monkeypatch.setenv('IGMC_GS_GRID', str(grid))
    else:
        monkeypatch.delenv('IGMC_GS_GRID', raising=False)
    if mute is None:
        monkeypatch.delenv('IGMC_EMU_FOLD_MUTE', raising=False)
    else:
        monkeypatch.setenv('IGMC_EMU_FOLD_MUTE', str(mute))
    g = engine.Graph(A, lib=lib)
    batch = engine.Batch(g, B, 1, cap)
    ws = engine.ModelWorkspace(lib, 0, R, 4, LABELS, 0, batch.node_capacity, batch.edge_capacity, B)
    P = PC.flatten_params(ws, PC.make_ref_model(LABELS, R, seed=4))
    M1, M2, G = np.zeros_like(P), np.zeros_like(P), np.zeros_like(P)
    out, loss, total = np.zeros(B, np.float32), np.zeros(2, np.float32), np.zeros(1, np.float64)
    ctrl = _ctrl_words(B)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    cp = vp(ctrl) if use_ctrl else None
    lib.call('igmc_batch_set_ctrl', batch.handle, cp)
    lib.call('igmc_model_set_ctrl', ws.handle, cp)
    engine.profile_fetch(lib)
    engine.profile_enable(lib, True)
    rec = []
    try:
        for i in range(steps):
            if use_ctrl:      # the cursor comes from the control block: selector = parity of the step
                batch.extract(lu, lv, ly, perm, i & 1, B, 1.0, 7, 999)
                if drop:
                    batch.edge_dropout(0.2, False, 7, i & 1)
            else:
                batch.extract(lu, lv, ly, perm, i * B, B, 1.0, 7, 3)
                if drop:
                    batch.edge_dropout(0.2, False, 7, (3 << 32) ^ i)
            lib.call('igmc_train_step', ws.handle, vp(P), batch.handle, int(drop), None, 7, 11 + i, 1.0, ARR, vp(out), vp(G),
                     vp(M1), vp(M2), vp(loss), vp(total), cp, i + 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, None)
            rec.append(dict(P=P.copy(), M1=M1.copy(), M2=M2.copy(), G=G.copy(), out=out.copy(), loss=loss.copy(),
                            total=total.copy(), ctrl=ctrl.copy(), img=_images(lib, ws)))
    finally:
        engine.profile_enable(lib, False)
        lib.call('igmc_batch_set_ctrl', batch.handle, None)
        lib.call('igmc_model_set_ctrl', ws.handle, None)
    labels = {n: c for n, _, c in engine.profile_fetch(lib)}
    return rec, labels, ws


#          B  cap cs grid drop   ARR    ctrl     slots of the partial tables
CASES = [(1, 8, 1, 0, False, 0.0, True),       # 1
         (7, 12, 2, 0, True, 0.001, True),     # 2 x 7 = 14 (< 16)
         (17, 16, 4, 0, True, 0.001, False),   # 4 x 17 = 68 (no multiple of 16)
         (50, 16, 4, 0, False, 0.001, True),   # 4 x 50 = 200
         (17, 12, 1, 5, True, 0.0, True),      # 5 workgroups walk 17 subgraphs
         (7, 8, 1, 0, True, 0.001, False)]     # 7, one workgroup per subgraph


@pytest.mark.parametrize('B,cap,cs,grid,drop,ARR,use_ctrl', CASES)
def test_one_launch_tail_leaves_the_bits_of_the_two_launch_tail(be, data, monkeypatch, B, cap, cs, grid, drop, ARR, use_ctrl):
    new, lab_new, ws = run_steps(be, data, monkeypatch, True, B, cap, cs, grid, drop, ARR, use_ctrl)
    be.lib.call('igmc_model_check', ws.handle, None)      # no bounded wait ran out
    old, lab_old, _ = run_steps(be, data, monkeypatch, False, B, cap, cs, grid, drop, ARR, use_ctrl)
    # the launches: the subgraph kernel and ONE tail launch a step -- against two with the switch off
    assert lab_new.get('k_tail_fin') == STEPS and 'k_tail_ts' not in lab_new and 'k_finalize_adam' not in lab_new, lab_new
    assert lab_old.get('k_tail_ts') == STEPS and lab_old.get('k_finalize_adam') == STEPS and 'k_tail_fin' not in lab_old, lab_old
    assert lab_new.get('k_graph_step') == STEPS and lab_old.get('k_graph_step') == STEPS
    for i, (a, b) in enumerate(zip(new, old)):
        for k in a:
            assert np.array_equal(a[k], b[k]), ('step', i, k)
        assert np.isfinite(a['P']).all() and np.isfinite(a['loss']).all()
    assert not np.array_equal(new[0]['P'], new[-1]['P'])
    if use_ctrl:
        assert new[-1]['ctrl'][_lib.CTRL['SYNC_ERR']] == 0 and new[-1]['ctrl'][_lib.CTRL['STEP']] == 11 + STEPS


def test_a_hand_off_that_never_arrives_leaves_its_layer_untouched_and_is_reported(be, data, monkeypatch):
    """Emulator only: the workgroups of conv layer 2 publish nothing, so the layer's words keep the tag they were initialised
    with.  Every workgroup of that layer gives up: its parameters and moments stay as they were, the other layers and lin1 / lin2
    take their step, and the step reports it -- sync_err bit 8 in the control block, and the model's check raises."""
    B = 7
    rec, labels, ws = run_steps(be, data, monkeypatch, True, B, 12, 2, 0, False, 0.001, True, steps=1, mute=2)
    assert labels.get('k_tail_fin') == 1
    lib = be.lib
    P0 = PC.flatten_params(ws, PC.make_ref_model(LABELS, R, seed=4))
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
