"""Checks of how the subgraph kernel (``k_graph_step2``) hands its partial weight-gradient tables to the tail, shared by
tests/test_emu_table_store.py (host emulation of the HIP sources) and tests/test_gpu_table_store.py (the gfx950 library).

The table product of backward layers 2 and 1 runs with its two operands swapped, so that a lane holds four consecutive
columns of one table row and stores a tile as one 16-byte store per lane -- written through to memory by the straight-line
forms --, and the 24 tiles are dealt to the waves so that a wave's first two fill whole lines.  What can go wrong is an
element of a slot that no store covers any more, a tile stored transposed or owned by two waves or none, a relation tile
``R <= r < G2_NR`` that is skipped (or not) on the wrong side of the swap, and the ``+=`` form of the looping grid.  So:

* extents 1 x 1 (no edge), 16 x 17 (a second bundle on one side only), 65 x 3 (a member with one active bundle; the other
  side's second member idle) and 101 x 101 as a cluster of 4 workgroups;
* the looping grid (``IGMC_GS_GRID`` below the batch size: a workgroup adds its later subgraphs to its slot with ``+=``) holds
  32 nodes a side, so it takes 1 x 1 and 16 x 17 and, in place of the two wider ones, their like within 32: 32 x 3 (one side
  full, the other one bundle) and 32 x 32, and 17 x 16 so that each of its two workgroups meets both parities;
* R = 5, and R = 2 (the tiles of relations 2 .. 4 are skipped);
* with and without edge dropout (injected flags).

Per case (``check_case``): one ``loss_grad`` and one ``igmc_train_step`` (Adam), each run TWICE from a workspace whose
tables, centre vectors and ``h_l`` rows were filled with different byte values (``igmc_debug_fill_tables``: 0xFF, NaNs, then
0x4B) -- the two runs must be bit-equal, which an element the stores miss cannot be.  Outputs, loss and every gradient tensor
are held to ``oracle/pyg_ref`` in float64 at the tolerances of tests/layer3_checks.py (``OUT_TOL`` / ``LOSS_RTOL`` /
``GRAD_TOL``); the Adam step's stored gradient likewise, and its parameters and moments to float64 Adam from that gradient
element by element (``adam_checks.adam_identity``)."""
import ctypes

import numpy as np

import adam_checks as AC
import history_checks as HC
import layer3_checks as L3
import parity_checks as PC

FILLS = (0xFF, 0x4B)
WG4 = [(1, 1), (16, 17), (65, 3), (101, 101)]
LOOP = [(1, 1), (16, 17), (17, 16), (32, 3), (32, 32)]
HYP = (HC.LR, 0.9, 0.999, 1e-8, 0.0)          # what history_checks.run_train_step passes


def _case(id, mnph, R, targets, expect):
    cap = mnph + 1
    assert all(max(t[:2]) <= cap for t in targets)
    return HC.Case(id, mnph, R, len(targets), (cap, cap), targets, expect)


_SUB4 = dict(family='subgraph', wg_per_graph=4)
_LOOP = dict(family='subgraph', wg_per_graph=1, loop=True)
ROWS = {
    'wg4_r5': (_case('table_store_wg4_r5', 127, 5, WG4, _SUB4), {'IGMC_GS_CLUSTER': '4'}),
    'wg4_r2': (_case('table_store_wg4_r2', 127, 2, WG4, _SUB4), {'IGMC_GS_CLUSTER': '4'}),
    # two workgroups for five subgraphs: workgroup 0 takes subgraphs 0, 2, 4, workgroup 1 takes 1, 3
    'loop_r5': (_case('table_store_loop_r5', 31, 5, LOOP, _LOOP), {'IGMC_GS_CLUSTER': '1', 'IGMC_GS_GRID': '2'}),
    'loop_r2': (_case('table_store_loop_r2', 31, 2, LOOP, _LOOP), {'IGMC_GS_CLUSTER': '1', 'IGMC_GS_GRID': '2'}),
}


def fill_tables(be, ws, byte):
    be.sync()
    be.lib.call('igmc_debug_fill_tables', ws.handle, ctypes.c_int(byte))


def _bit_equal(a, b, keys, what):
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.tobytes() == y.tobytes(), '%s: %s is not bit-equal (%d of %d entries differ)' % (
            what, k, int((x.view(np.uint32) != y.view(np.uint32)).sum()), x.size)


def _train_step(cr, b, ws, bufs, drop):
    res = HC.run_train_step(cr, b, ws, bufs, cr.target, drop)
    res['grad'] = cr.be.host(bufs.G)
    return res


def oracle_grads(cr, d, drop):
    """The float64 gradient tensors of the target batch (``oracle/pyg_ref``)."""
    import torch
    from helpers import batch_to_pyg
    from oracle import pyg_ref
    edge_mask = torch.from_numpy((HC.edge_flags_by_id(d) & 1).astype(bool)) if drop else None
    lin_mask = torch.from_numpy(cr.lin[cr.target])
    m = PC.make_ref_model(cr.L, cr.case.R, seed=3, adj_dropout=0.2 if drop else 0.0).to(torch.float64)
    pyg = batch_to_pyg(d, cr.L)
    pyg.x, pyg.y = pyg.x.to(torch.float64), pyg.y.to(torch.float64)
    rl, ro, rg = pyg_ref.loss_and_grads(m, pyg, ARR=HC.ARR, edge_mask=edge_mask, lin_mask=lin_mask)
    return float(rl), ro.numpy().astype(np.float64), {k: v.numpy().astype(np.float64) for k, v in rg.items()}


def check_case(cr, drop):
    be, B, id = cr.be, cr.case.B, cr.case.id
    # ---- loss_grad, twice, from differently filled workspaces
    b, ws = cr.pair()
    runs = []
    for byte in FILLS:
        fill_tables(be, ws, byte)
        res = HC.run_step(cr, b, ws, cr.target, drop)
        HC.assert_finite(res, '%s: loss_grad on a workspace filled with 0x%02X' % (id, byte))
        runs.append(res)
    assert cr.geometry is not None
    HC.same_batch(runs[0]['d'], runs[1]['d'])
    _bit_equal(runs[0], runs[1], ('ev', 'out', 'loss', 'grad'), id + ': loss_grad from workspaces filled with 0xFF and 0x4B')
    L3.check_named_oracle(cr, runs[0], drop)
    # ---- one step with Adam, twice likewise (the caller restores its own buffers in place in between)
    b, ws = cr.pair()
    bufs = HC.TrainBufs(cr, ws)
    steps = []
    for byte in FILLS:
        bufs.restore(be)
        fill_tables(be, ws, byte)
        steps.append(_train_step(cr, b, ws, bufs, drop))
    keys = ('out', 'loss', 'grad', 'params', 'm1', 'm2')
    _bit_equal(steps[0], steps[1], keys, id + ': train step from workspaces filled with 0xFF and 0x4B')
    t = steps[0]
    rl, ro, rg = oracle_grads(cr, runs[0]['d'], drop)
    grads = PC.unflatten_grads(ws, t['grad'])
    bad = []
    for k in sorted(rg):
        e = float(np.abs(grads[k] - rg[k]).max() / max(np.abs(rg[k]).max(), 1e-6))
        print('%s drop=%s train step grad %-16s rel err %.3e' % (id, drop, k, e))
        if not e < PC.GRAD_TOL:
            bad.append('gradient of %s: %.3e' % (k, e))
    assert not bad, '%s (extents %s, dropout %s): the train step\'s gradient beyond GRAD_TOL %.1e vs the float64 oracle -- %s' % (
        id, cr.case.targets, drop, PC.GRAD_TOL, '; '.join(bad))
    e_out = PC.rel_err(HC._outputs(t['out'], B, id + ' (train step)'), ro)
    e_loss = abs(float(t['loss'][0]) - rl) / max(abs(rl), 1e-12)
    print('%s drop=%s train step out %.3e loss %.3e' % (id, drop, e_out, e_loss))
    assert e_out < PC.OUT_TOL, '%s: train step outputs %.3e vs the oracle' % (id, e_out)
    assert e_loss < PC.LOSS_RTOL, '%s: train step loss %.3e vs the oracle' % (id, e_loss)
    zero = np.zeros_like(cr.flat)
    AC.adam_identity(cr.flat, zero, zero, t['grad'], t['params'], t['m1'], t['m2'], 1, HYP, what=id + ' (train step)')
