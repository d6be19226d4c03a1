"""Checks of conv layer 3 in the subgraph kernel (``k_graph_step2``), shared by tests/test_emu_layer3.py (host emulation of
the HIP sources) and tests/test_gpu_layer3.py (the gfx950 library).

The readout takes ``h_3`` of the two target rows only, so the kernel runs layer 3's forward on the two centre bundles alone
and its backward in closed form: ``dPre_3`` lives on the two centre rows, ``dX[j]`` is one of five vectors
``g_r = dPre_3[c_opp] @ W_r^T`` chosen by the relation of the kept edge ``j -> c_opp``, and the layer's weight-gradient
table is two rank-1 products written by the workgroups that own a centre (exact zeros by every other one).  What can go
wrong is a matter of extents, ownership and keep bits, so the batches are crafted (``history_checks.crafted_graph``):

* sides (1,1) -- no edge at all --, (1,17) / (17,1) -- a centre whose bundle has one row --, (16,16) / (17,33) -- both sides
  of the 16-row bundle boundary --, (64,65) / (65,64) / (101,101) -- both sides of the 64-row workgroup boundary, where
  members without a centre are active and must write zero tables;
* R = 5, and R = 3 (relations 3 and 4 absent);
* with and without edge dropout, under injected flags in which edges incident to a centre keep every combination of
  directions in turn (``centre_flags``: a wrong keep bit cannot pass);
* clusters of 4, 2 and 1 workgroups and the looping single-workgroup grid (the ``+=`` table path), each with the shapes
  its slots hold; the geometry is asserted before any number (``Crafted.assert_geometry``).

Per case and mask form (``check_case``): outputs, loss and every gradient tensor against ``oracle/pyg_ref`` in float64 at
the suite's ``OUT_TOL`` / ``LOSS_RTOL`` / ``GRAD_TOL`` (``convs.3`` and ``convs.2`` named in the failure); the target batch
after a batch that filled every slot of the same arena and workspace value-equal to the target batch on new memory; two
launches on the same inputs bit-equal.  The evaluation variant (``TRAIN = false``) and the training launch apply different
heads by design (MLP dropout), so their outputs are not comparable to each other: each is held to the oracle's output of
the same forward at ``OUT_TOL``, on the same batch."""
import numpy as np

import history_checks as HC
import parity_checks as PC

_BY_ID = HC.edge_flags_by_id
SHAPES = [(1, 1), (1, 17), (17, 1), (16, 16), (17, 33), (64, 65), (65, 64), (101, 101)]


def _fit(cap):
    return [s for s in SHAPES if max(s) <= cap]


def _case(id, mnph, R, targets, expect):
    cap = mnph + 1
    assert all(max(t[:2]) <= cap for t in targets)
    return HC.Case(id, mnph, R, len(targets), (cap, cap), targets, expect)


# One row per launch structure: the arena's slot extent selects what the cluster hook may take (4 workgroups: <= 128 a side,
# 2: <= 64, 1: <= 32); every row takes all the shapes its slots hold, the smaller slots a few of their own on both sides of
# their bundle and workgroup boundaries.  ``env``: the hooks of tests/geometry_cases.py.
ROWS = {
    'wg4': (_case('layer3_wg4', 127, 5, _fit(128), dict(family='subgraph', wg_per_graph=4)), {'IGMC_GS_CLUSTER': '4'}),
    'wg4_r3': (_case('layer3_wg4_r3', 127, 3, _fit(128), dict(family='subgraph', wg_per_graph=4)), {'IGMC_GS_CLUSTER': '4'}),
    'wg2': (_case('layer3_wg2', 63, 5, _fit(64) + [(33, 64), (64, 17), (49, 48)], dict(family='subgraph', wg_per_graph=2)),
            {'IGMC_GS_CLUSTER': '2'}),
    'wg1': (_case('layer3_wg1', 31, 5, _fit(32) + [(32, 17), (17, 32)], dict(family='subgraph', wg_per_graph=1)),
            {'IGMC_GS_CLUSTER': '1'}),
    # two workgroups for eight subgraphs: workgroup w takes subgraphs w, w + 2, .. and accumulates its tables with +=
    'wg1_loop': (_case('layer3_wg1_loop', 31, 5, _fit(32) + [(32, 17), (17, 32), (1, 32), (31, 2)],
                       dict(family='subgraph', wg_per_graph=1, loop=True)), {'IGMC_GS_CLUSTER': '1', 'IGMC_GS_GRID': '2'}),
}


def centre_flags(d, p=0.2, seed=77):
    """``history_checks.edge_flags_by_id`` with the edges incident to a target node overridden: edge (u, v) keeps
    (both, item -> user only, user -> item only, neither) for (u + v) % 4 = 0 .. 3 -- a function of the global ids, like the
    rest.  Entry of the dst-sorted CSR: bit 0 = keep(src -> dst), bit 1 = keep(dst -> src)."""
    fl = _BY_ID(d, p, seed)
    N = d['N']
    dst = np.repeat(np.arange(N, dtype=np.int64), np.diff(d['row_ptr']).astype(np.int64))
    src = d['col'].astype(np.int64)
    lab = d['node_label']
    row_user = lab[dst] % 2 == 0
    gd, gs = d['node_gid'][dst].astype(np.int64), d['node_gid'][src].astype(np.int64)
    u, v = np.where(row_user, gd, gs), np.where(row_user, gs, gd)
    pat = (u + v) % 4
    k_iu = np.isin(pat, (0, 1)).astype(np.uint8)          # item -> user kept
    k_ui = np.isin(pat, (0, 2)).astype(np.uint8)          # user -> item kept
    into_user = row_user                                   # src -> dst runs item -> user
    forced = np.where(into_user, k_iu | (k_ui << 1), k_ui | (k_iu << 1)).astype(np.uint8)
    centre = (lab[dst] <= 1) | (lab[src] <= 1)
    return np.where(centre, forced, fl).astype(np.uint8)


class flags_injected(object):
    """While active, every run of history_checks (engine and oracle alike) takes ``centre_flags``."""

    def __enter__(self):
        HC.edge_flags_by_id = centre_flags

    def __exit__(self, *exc):
        HC.edge_flags_by_id = _BY_ID


def assert_one_way_centre_edges(d):
    """The injected flags do hold centre edges that keep exactly one direction, of both kinds (where the batch has edges)."""
    N = d['N']
    dst = np.repeat(np.arange(N, dtype=np.int64), np.diff(d['row_ptr']).astype(np.int64))
    lab = d['node_label']
    centre = (lab[dst] <= 1) | (lab[d['col'].astype(np.int64)] <= 1)
    fl = centre_flags(d)[centre]
    assert (fl == 1).any() and (fl == 2).any(), 'no centre edge keeps exactly one direction'


def check_named_oracle(cr, res, drop):
    """Every gradient tensor, the outputs of both variants and the loss against ``oracle/pyg_ref`` in float64, the layer-3
    and layer-2 tensors first and by name."""
    import torch
    from helpers import batch_to_pyg
    from oracle import pyg_ref
    d, B = res['d'], len(res['order'])
    edge_mask = torch.from_numpy((HC.edge_flags_by_id(d) & 1).astype(bool)) if drop else None
    lin_mask = torch.from_numpy(cr.lin[res['order']])
    m = PC.make_ref_model(cr.L, cr.case.R, seed=3, adj_dropout=0.2 if drop else 0.0).to(torch.float64)
    pyg = batch_to_pyg(d, cr.L)
    pyg.x, pyg.y = pyg.x.to(torch.float64), pyg.y.to(torch.float64)
    _, ev = pyg_ref.eval_sse(m, pyg)
    rl, ro, rg = pyg_ref.loss_and_grads(m, pyg, ARR=HC.ARR, edge_mask=edge_mask, lin_mask=lin_mask)
    grads = PC.unflatten_grads(res['ws'], res['grad'])
    keys = sorted(rg, key=lambda k: (not k.startswith('convs.3'), not k.startswith('convs.2'), k))
    for want in ('convs.3.basis', 'convs.3.att', 'convs.3.root', 'convs.3.bias', 'convs.2.basis', 'convs.2.att',
                 'convs.2.root', 'convs.2.bias'):
        assert want in rg and want in grads, (want, sorted(rg))
    errs = {}
    for k in keys:
        r = rg[k].numpy().astype(np.float64)
        errs[k] = float(np.abs(grads[k] - r).max() / max(np.abs(r).max(), 1e-6))
        print('%s drop=%s grad %-16s rel err %.3e' % (cr.case.id, drop, k, errs[k]))
    e_ev = PC.rel_err(res['ev'][:B], ev.numpy().astype(np.float64))
    e_out = PC.rel_err(res['out'][:B], ro.numpy().astype(np.float64))
    e_loss = abs(float(res['loss'][0]) - float(rl)) / max(abs(float(rl)), 1e-12)
    print('%s drop=%s eval out %.3e train out %.3e loss %.3e' % (cr.case.id, drop, e_ev, e_out, e_loss))
    bad = ['gradient of %s: %.3e' % (k, errs[k]) for k in keys if not errs[k] < PC.GRAD_TOL]
    assert not bad, '%s (extents %s, dropout %s): beyond GRAD_TOL %.1e vs the float64 oracle -- %s' % (
        cr.case.id, cr.case.targets, drop, PC.GRAD_TOL, '; '.join(bad))
    assert e_ev < PC.OUT_TOL, '%s: evaluation variant (TRAIN = false) outputs %.3e vs the oracle' % (cr.case.id, e_ev)
    assert e_out < PC.OUT_TOL, '%s: training outputs %.3e vs the oracle' % (cr.case.id, e_out)
    assert e_loss < PC.LOSS_RTOL, '%s: loss %.3e vs the oracle' % (cr.case.id, e_loss)
    return errs


def assert_bit_equal(a, b, what):
    for k in ('ev', 'out', 'loss', 'grad'):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.tobytes() == y.tobytes(), '%s: %s is not bit-equal (%d of %d entries differ)' % (
            what, k, int((x.view(np.uint32) != y.view(np.uint32)).sum()), x.size)


def check_case(cr, drop):
    """All of the module docstring for one row and mask form.  (``Crafted.assert_geometry`` runs inside every step, before
    its numbers are looked at.)"""
    with flags_injected():
        h0 = cr.h0(drop)                                   # the target batch on a new arena and a new workspace
        assert cr.geometry is not None
        if drop:
            assert_one_way_centre_edges(h0['d'])
        b, ws = cr.pair()
        HC.run_step(cr, b, ws, cr.dirty, drop, exact_flags=False)      # every slot filled to its full extent
        h1 = HC.run_step(cr, b, ws, cr.target, drop)
        HC.same_batch(h0['d'], h1['d'])
        HC.assert_same(h0, h1, cr.case.id + ': after a batch that filled every slot vs new memory')
        h2 = HC.run_step(cr, b, ws, cr.target, drop)       # the same launches again on the same arena and workspace
        assert_bit_equal(h1, h2, cr.case.id + ': second launch on the same inputs')
        errs = check_named_oracle(cr, h1, drop)
        HC.check_oracle(cr, h1, drop)                      # (the suite's own summary record, same tolerances)
    return errs
