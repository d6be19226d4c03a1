"""Checks of what the subgraph kernel's head leaves behind under clusters of workgroups (g2_subgraph.h), shared by the emulator test
(tests/test_emu_head_split.py) and the GPU test (tests/test_gpu_head_split.py)."""
import ctypes

import numpy as np

HEAD_ARRAYS = dict(a1=0, dz=1, feat=2, gfeat=3)


def head_arrays(be, ws, B):
    """Host copies of what the head of the last training launch left: a1 / dz [B, 128], feat / gfeat [B, 256], lmask [B, 128]."""
    be.sync()
    res = {}
    for key, which in HEAD_ARRAYS.items():
        w = 128 if which < 2 else 256
        buf = np.full(B * w, np.nan, np.float32)
        be.lib.call('igmc_debug_head_array', ws.handle, which, ctypes.c_void_p(buf.ctypes.data), B * w)
        res[key] = buf.reshape(B, w)
    lm = np.full(B * 128, 255, np.uint8)
    be.lib.call('igmc_debug_lin_mask', ws.handle, ctypes.c_void_p(lm.ctypes.data), B * 128)
    res['lmask'] = lm.reshape(B, 128)
    return res


def check_head_arrays(arr, res, multiply_by=1.0):
    """Every hidden unit of every subgraph written, by whichever member owns it: the arrays against a float64 restatement
    of the head on the kernel's own readout ``feat`` (whose correctness the d lin1 / d lin2 parity of
    ``run_model_parity`` covers) -- a unit nobody wrote, or one written from another unit's values, fails here.
    Bounds: f32 dot products of 256 / 128 terms, 1e-5 of the array's peak."""
    sd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in res['ref'].state_dict().items()}
    W1, b1, w2 = sd['lin1.weight'], sd['lin1.bias'], sd['lin2.weight'].reshape(-1)
    B = res['d']['B']
    feat = arr['feat'].astype(np.float64)
    for key in ('a1', 'dz', 'feat', 'gfeat'):
        assert np.isfinite(arr[key]).all(), key
    assert np.ptp(feat) > 0
    mask = res['lin_mask']
    assert np.array_equal(arr['lmask'], mask.astype(np.uint8)), 'lmask is not the injected mask'
    a1 = np.maximum(feat @ W1.T + b1, 0.0)

    def close(got, want, what):
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-12)
        assert err < 1e-5, '%s: max error relative to the peak %.3e' % (what, err)
    close(arr['a1'], a1, 'a1')
    y = np.asarray(res['d']['y'], np.float64)[:B]
    dp = 2.0 * (res['train_out'].astype(np.float64) - y) * (1.0 / B) * multiply_by
    live = (arr['a1'] > 0) & mask                 # (the kernel's own ReLU decision: a unit within rounding of 0 may differ)
    for c in range(4):                            # (every member's units of a cluster of four carry gradient somewhere)
        assert live[:, 32 * c:32 * c + 32].any(), c
    dz = dp[:, None] * live * 2.0 * w2[None, :]
    close(arr['dz'], dz, 'dz')
    assert np.array_equal(arr['dz'] != 0, live & (dp[:, None] != 0) & (w2[None, :] != 0))
    close(arr['gfeat'], dz @ W1, 'gfeat')


def relaunch(be, res, use_dropout, multiply_by=1.0, ARR=0.001):
    """The training launch of ``run_model_parity`` once more on the same inputs: outputs, loss, gradients, head arrays."""
    ws, b, B = res['ws'], res['batch'], res['d']['B']
    lm = be.dev(res['lin_mask'].astype(np.uint8).reshape(-1))
    out, grad, loss = be.dev(np.zeros(B, np.float32)), be.dev(np.zeros(ws.n_params, np.float32)), be.dev(np.zeros(2, np.float32))
    ws.loss_grad(be.ptr(res['P']), b, be.ptr(out), be.ptr(grad), be.ptr(loss), use_edge_flags=use_dropout,
                 lin_mask=be.ptr(lm), multiply_by=multiply_by, ARR=ARR)
    got = dict(out=be.host(out), grad=be.host(grad), loss=be.host(loss))
    got.update(head_arrays(be, ws, B))
    return got


def check_bit_identical(r1, r2):
    for k in sorted(r1):
        assert np.array_equal(r1[k], r2[k]), '%s differs between two launches on the same inputs' % k


def check_error_word(be, ws):
    """``igmc_model_check`` fails when a bounded device-side wait (plane flags, readout words) timed out."""
    be.lib.call('igmc_model_check', ws.handle, None)
