"""Checks of conv layer 3's forward in closed form (``k_graph_step2``, igmc_amd/csrc/g2_subgraph.h), shared by
tests/test_emu_l3_forward.py (host emulation of the HIP sources) and tests/test_gpu_l3_forward.py (the gfx950 library).

The readout takes ``h_3`` of the two target rows only.  Their aggregates ``T_r[c] = sum_j h_2[j]`` over the opposite side's rows
``j`` whose kept edge ``j -> c`` has relation ``r`` are summed where ``h_2`` is formed -- layer 2's epilogue, per 16-row bundle --
and cross the workgroups as tagged words; every member of a cluster adds the bundles and forms ``h_3`` of both centres with
five 32 x 32 matvecs a side.  What can go wrong is the relation and keep bit a row reads, the bundle a word belongs to, a word
an earlier launch left, and a member that reads before a producer wrote -- so the batches are the crafted ones of
``layer3_checks`` (``ROWS``: every launch structure, R = 5 and 3, the shapes on both sides of the bundle and workgroup
boundaries) with and without ``centre_flags``.

1. ``check_sums``: the summed ``T_r[c]`` the training launch left (``igmc_debug_l3_sums``: rows r < R of the centre vectors)
   against the float64 sum of the kernel's OWN stored ``h_2`` rows over the rows the batch's relations and flags select.  Bound
   per entry: ``(n - 1) 2^-24 sum_j |h_2[j][f]|`` -- the first-order bound of ANY order of n float32 additions -- plus one ulp of
   the result; a centre without a kept neighbour of the relation, and the rows of absent relations (R = 3), are exact zeros.  With
   the keep bit of the other direction the same comparison must fail.
2. ``check_stale``: (17,33) and (1,1) after (101,101) -- every bundle's words written -- on the same arena and workspace, value-equal
   to new memory; the same launch twice, bit-equal.
3. ``check_eval``: the evaluation kernel's and the training launch's outputs against the oracle's forward at ``OUT_TOL``.
4. the head's arrays with the lin1 rows requested early: ``head_split_checks.check_head_arrays`` (in the test files)."""
import ctypes

import numpy as np

import history_checks as HC
import layer3_checks as L3
import parity_checks as PC

NR = 5                      # G2_NR: relation rows of a centre's vectors; rows NR, NR + 1 are h_2[c] and dPre_3[c]
SUM_ROWS = ('wg4', 'wg4_r3', 'wg2')      # clustered steps: the launches that leave centre vectors
STALE = HC.Case('l3_forward_stale', 127, 5, 2, (101, 101), [(17, 33), (1, 1)], dict(family='subgraph', wg_per_graph=4))
STALE_ENV = {'IGMC_GS_CLUSTER': '4'}

_RUNS = {}


def run(cr, name, drop):
    """The row's target batch on a new arena and workspace under ``centre_flags`` (once per row and mask form, shared)."""
    if (name, drop) not in _RUNS:
        with L3.flags_injected():
            b, ws = cr.pair()
            res = HC.run_step(cr, b, ws, cr.target, drop)
            HC.assert_finite(res, name)
            cr.be.lib.call('igmc_model_check', ws.handle, None)      # no bounded wait ran out
            res['b'] = b
            res['flags'] = HC.edge_flags_by_id(res['d']) if drop else None
        _RUNS[(name, drop)] = res
    return _RUNS[(name, drop)]


def l3_sums(be, ws, b, B):
    """-> (centre vectors [B, 2, NR + 2, 32], stored h_2 rows [B, 2, 128, 32]) of the last training launch"""
    be.sync()
    vec = np.full(B * 2 * (NR + 2) * 32, np.nan, np.float32)
    h2 = np.zeros(B * 2 * 128 * 32, np.float32)
    for which, buf in ((0, vec), (1, h2)):
        be.lib.call('igmc_debug_l3_sums', ws.handle, b.handle, ctypes.c_int(which), ctypes.c_void_p(buf.ctypes.data),
                    ctypes.c_int64(buf.size))
    return vec.reshape(B, 2, NR + 2, 32), h2.reshape(B, 2, 128, 32)


def expected_sums(d, h2, flags, keep_bit=0):
    """float64 ``T_r[c]`` of both centres of every subgraph from the stored ``h_2`` rows: over the centre's CSR row (its
    in-edges ``src -> c``), kept where bit ``keep_bit`` of the entry's flags says so (bit 0 = keep(src -> dst): the right one).
    -> (T [B, 2, NR, 32], sum of |terms| alike, terms [B, 2, NR])"""
    B, off, nu = d['B'], d['node_off'], d['n_users']
    T, A, n = np.zeros((B, 2, NR, 32)), np.zeros((B, 2, NR, 32)), np.zeros((B, 2, NR), np.int64)
    for g in range(B):
        for sd in (0, 1):
            c = int(off[g]) + (int(nu[g]) if sd else 0)
            assert d['node_label'][c] == sd, 'row %d is not the centre of side %d' % (c, sd)
            for e in range(int(d['row_ptr'][c]), int(d['row_ptr'][c + 1])):
                if flags is not None and not (int(flags[e]) >> keep_bit) & 1:
                    continue
                j = int(d['col'][e]) - int(off[g])
                sj, ij = (0, j) if j < nu[g] else (1, j - int(nu[g]))
                assert sj == 1 - sd and 0 <= ij < 128
                r = int(d['erel'][e])
                row = h2[g, sj, ij].astype(np.float64)
                T[g, sd, r] += row
                A[g, sd, r] += np.abs(row)
                n[g, sd, r] += 1
    return T, A, n


def compare_sums(vec, T, A, n, R, what):
    """-> the largest error as a share of its bound (entries with a bound of zero must be exact)."""
    got = vec[:, :, :NR, :].astype(np.float64)
    assert np.isfinite(got).all(), '%s: non-finite centre sums' % what
    assert not got[:, :, R:, :].any(), '%s: rows of absent relations are not exact zeros' % what
    empty = n == 0
    assert not got[empty].any(), '%s: a centre without a kept neighbour of the relation is not exact zeros' % what
    ulp = np.spacing(np.abs(T).astype(np.float32)).astype(np.float64)
    bound = np.maximum(n - 1, 0)[..., None] * 2.0 ** -24 * A + np.where(empty[..., None], 0.0, ulp)
    err = np.abs(got - T)
    bad = err > bound
    worst = float((err[~empty] / bound[~empty]).max()) if (~empty).any() else 0.0
    assert not bad.any(), '%s: %d centre sums beyond (n - 1) 2^-24 sum|h_2| + 1 ulp (first at [graph, side, r, f] = %s: %.3e vs %.3e)' % (
        what, int(bad.sum()), np.argwhere(bad)[0].tolist(), float(err[bad][0]), float(bound[bad][0]))
    return worst


def check_sums(cr, name, drop):
    res = run(cr, name, drop)
    d, ws, B, R = res['d'], res['ws'], cr.case.B, cr.case.R
    assert ws.l3_vectors(res['b'], B) != 0, '%s: the step does not leave centre vectors' % name
    vec, h2 = l3_sums(cr.be, ws, res['b'], B)
    got_h2c = vec[:, :, NR, :]
    own = np.stack([h2[:, 0, 0, :], h2[:, 1, 0, :]], 1)
    assert np.array_equal(got_h2c, own), '%s: row G2_NR of the centre vectors is not the stored h_2 of the centre row' % name
    assert np.ptp(h2) > 0
    worst = compare_sums(vec, *expected_sums(d, h2, res['flags']), R, '%s drop=%s' % (name, drop))
    shapes = [(int(a), int(b1 - b0 - a)) for a, b0, b1 in zip(d['n_users'], d['node_off'][:-1], d['node_off'][1:])]
    assert (1, 1) in shapes                                     # (a centre with no neighbour at all is among the cases)
    print('%s drop=%s centre sums: worst error / bound %.3f' % (name, drop, worst))
    PC.record_observed('l3_forward_sums', case=name, backend=cr.be.name, dropout=bool(drop), worst_err_over_bound=worst)
    if drop:
        L3.assert_one_way_centre_edges(d)
        try:
            compare_sums(vec, *expected_sums(d, h2, res['flags'], keep_bit=1), R, 'other direction')
        except AssertionError:
            pass
        else:
            raise AssertionError('%s: the sums also match the keep bit of the other direction: the check cannot see it' % name)
    return worst


def check_stale(cr, drop):
    """(17,33) and (1,1) after (101,101) on the same arena and workspace; the same launch twice."""
    with L3.flags_injected():
        h0 = cr.h0(drop)
        b, ws = cr.pair()
        HC.run_step(cr, b, ws, cr.dirty, drop, exact_flags=False)      # every bundle of both sides leaves its words
        h1 = HC.run_step(cr, b, ws, cr.target, drop)
        HC.same_batch(h0['d'], h1['d'])
        HC.assert_same(h0, h1, 'after (101,101) on the same arena and workspace vs new memory')
        h2 = HC.run_step(cr, b, ws, cr.target, drop)
        L3.assert_bit_equal(h1, h2, 'second launch on the same inputs')
        cr.be.lib.call('igmc_model_check', ws.handle, None)


def check_eval(cr, name, drop):
    """Outputs of the evaluation kernel (``TRAIN = false``) and of the training launch against the oracle's forward of the
    same batch in float64 at ``OUT_TOL``."""
    import torch
    from helpers import batch_to_pyg
    from oracle import pyg_ref
    res = run(cr, name, drop)
    d, B = res['d'], cr.case.B
    m = PC.make_ref_model(cr.L, cr.case.R, seed=3, adj_dropout=0.2 if drop else 0.0).to(torch.float64)
    pyg = batch_to_pyg(d, cr.L)
    pyg.x, pyg.y = pyg.x.to(torch.float64), pyg.y.to(torch.float64)
    _, ev = pyg_ref.eval_sse(m, pyg)
    edge_mask = torch.from_numpy((res['flags'] & 1).astype(bool)) if drop else None
    _, ro, _ = pyg_ref.loss_and_grads(m, pyg, ARR=HC.ARR, edge_mask=edge_mask, lin_mask=torch.from_numpy(cr.lin[res['order']]))
    e_ev = PC.rel_err(res['ev'][:B], ev.numpy().astype(np.float64))
    e_out = PC.rel_err(res['out'][:B], ro.numpy().astype(np.float64))
    print('%s drop=%s eval out %.3e train out %.3e' % (name, drop, e_ev, e_out))
    PC.record_observed('l3_forward_outputs', case=name, backend=cr.be.name, dropout=bool(drop), eval_out_rel=e_ev, train_out_rel=e_out)
    assert e_ev < PC.OUT_TOL, '%s: evaluation kernel outputs %.3e vs the oracle' % (name, e_ev)
    assert e_out < PC.OUT_TOL, '%s: training outputs %.3e vs the oracle' % (name, e_out)
    return e_ev, e_out
