"""History and position checks of the model step, shared by tests/test_emu_history.py (host emulation of the HIP sources)
and tests/test_gpu_history.py (the gfx950 library).

Every other parity test extracts one batch into a brand-new arena and runs it on a brand-new workspace.  A training run
re-fills the same arenas and one workspace serves every step, and the kernels lean on what earlier launches left behind:
``k_extract_nodes`` clears only the rows a subgraph occupies, ``k_graph_step2`` loads block bytes unguarded and masks
afterwards, the plane images in LDS and in the exchange regions are never cleared (``0 * stale == 0``), idle bundles must
leave exact zeros.  Here a batch of subgraphs of exactly chosen extents -- 1 x 1, 1 x full, extents on both sides of every
8 / 16 / 32 / 64 boundary the masks are written for -- runs after a batch that filled every slot to its full extent, and
must give the very values it gives on new memory; each subgraph's outputs must not depend on where in the batch it sits or
on its batch-mates; and the result is held to ``oracle/pyg_ref`` in float64.

The rating graphs are crafted (``crafted_graph``): disjoint blocks, one per link, so that the uncapped hop-1 extraction of
block i's link yields exactly ``n_u x n_v`` nodes through the real extraction kernels."""
import collections

import numpy as np
import scipy.sparse as ssp

import parity_checks as PC
from helpers import batch_to_pyg
from igmc_amd import engine

ARR = 0.001
LR = 1e-3
OUT_PAD = 8          # NaN sentinels behind the outputs of a batch: no launch may touch them


# ====================================================================== crafted rating graphs
def crafted_graph(blocks, R):
    """Rating matrix of disjoint blocks, one per link.  ``blocks``: ``[(n_u, n_v, density)]``.  Block i has ``n_u`` users and
    ``n_v`` items; its target user (the block's first) rates every item of the block and every user of the block rates the
    target item (the block's first); the remaining pairs are rated with probability ``density``; ratings cycle through all
    ``R`` relations.  The uncapped hop-1 subgraph of link ``(U_i[0], V_i[0])`` is then the whole block: exactly ``n_u`` user
    and ``n_v`` item nodes (a ``(1, 1)`` block: an edgeless pair -- the link's own rating is removed).
    -> (csr matrix with values 1 .. R, links [n, 2])"""
    rng = np.random.default_rng(20)
    rows, cols, vals, links = [], [], [], []
    u0 = v0 = 0
    for k, (nu, nv, dens) in enumerate(blocks):
        m = rng.random((nu, nv)) < dens
        m[0, :] = True
        m[:, 0] = True
        i, j = np.nonzero(m)
        rows.append(u0 + i)
        cols.append(v0 + j)
        vals.append(1 + (i * nv + j + k) % R)
        links.append((u0, v0))
        u0 += nu
        v0 += nv
    A = ssp.csr_matrix((np.concatenate(vals).astype(np.float32), (np.concatenate(rows), np.concatenate(cols))),
                       shape=(u0, v0))
    return A, np.array(links, np.int64)


def _block(t, default_density=0.6):
    return (int(t[0]), int(t[1]), float(t[2]) if len(t) > 2 else default_density)


def cycle(shapes, n):
    return [shapes[i % len(shapes)] for i in range(n)]


Case = collections.namedtuple('Case', 'id mnph R B full targets expect')

_DENSE = [(1, 1), (1, 201), (201, 1), (129, 127), (128, 130), (145, 17), (201, 201, 0.3)]
_WG1 = [(1, 1), (1, 32), (32, 1), (2, 3), (17, 15), (9, 28)]

# One row per step family: the arena's slot extent (``mnph`` + 1 a side, asserted through the geometry every run reports),
# the batch size that selects the family, the extent ``full`` of every block of the DIRTY batch (density 1) and the extents
# of the TARGET batch: both extents cover every residue mod 8 and both sides of 16 / 32 / 64 / 96 in the first row; 1 x 1,
# 1 x full and full x 1 in every row.
CASES = [
    Case('subgraph_wg4', 127, 5, 12, (128, 128),
         [(1, 1), (1, 128), (128, 1), (2, 3), (16, 16), (17, 15), (33, 31), (37, 5), (65, 63), (100, 36), (22, 94),
          (128, 127)], dict(family='subgraph', wg_per_graph=4)),
    Case('subgraph_wg2', 63, 5, 57, (64, 64),
         cycle([(1, 1), (1, 64), (64, 1), (33, 31), (17, 47), (9, 60), (64, 63)], 57), dict(family='subgraph', wg_per_graph=2)),
    # one workgroup per subgraph on a grid of 64 looping over 130 subgraphs: workgroup w takes slots w, w + 64, w + 128, so a
    # small subgraph follows a full one (and a full one a small one) in the same workgroup's LDS
    Case('subgraph_wg1_loop', 31, 5, 130, (32, 32),
         [(32, 32, 1.0)] * 64 + cycle(_WG1, 64) + [(32, 32, 1.0)] * 2, dict(family='subgraph', wg_per_graph=1, loop=True)),
    Case('dense_fused', 200, 5, 7, (201, 201), _DENSE, dict(family='dense_fused', dl_bwd=1, groups=1)),
    Case('dense_layer_tables', 200, 5, 57, (201, 201), cycle(_DENSE, 57), dict(family='dense_layer', tables=1)),
    Case('dense_layer_no_tables', 200, 5, 65, (201, 201), cycle(_DENSE, 65), dict(family='dense_layer', tables=0)),
    Case('r10_gsplit', 100, 10, 7, (101, 101),
         [(1, 1), (1, 101), (101, 1), (17, 15), (65, 63), (97, 33), (101, 101, 0.5)],
         dict(family='dense_fused', groups=2, gsplit=1)),
    Case('rows', 243, 5, 4, (244, 244), [(1, 1), (244, 3), (2, 244), (130, 129)], dict(family='rows')),
]
BY_ID = {c.id: c for c in CASES}


def smaller(case, B, pick=None):
    """The case at a smaller batch size (the emulator's runs): targets ``pick`` (indices) or the first ``B``."""
    pick = list(range(B)) if pick is None else list(pick)
    assert len(pick) == B
    return case._replace(B=B, targets=[case.targets[i] for i in pick])


# ====================================================================== one crafted case on a backend
def _assign(be, buf, arr):
    """In-place overwrite of a device buffer (what a caller restoring a checkpoint into its own buffers does)."""
    if be.name == 'emu':
        buf[...] = arr
    else:
        buf.copy_(be.torch.from_numpy(np.ascontiguousarray(arr)))


class Crafted(object):
    """Graph, links and reference model of a case.  Links ``0 .. B-1`` are the dirty batch, ``B .. 2B-1`` the target."""

    def __init__(self, be, case):
        self.be, self.case = be, case
        B = case.B
        blocks = [(case.full[0], case.full[1], 1.0)] * B + [_block(t) for t in case.targets]
        self.blocks = blocks
        A, links = crafted_graph(blocks, case.R)
        self.g = engine.Graph(A, device=be.device, lib=be.lib)
        self.lu, self.lv = be.dev(links[:, 0].astype(np.int32)), be.dev(links[:, 1].astype(np.int32))
        self.ly = be.dev((1 + np.arange(len(links)) % case.R).astype(np.float32))
        self.dirty, self.target = np.arange(B), B + np.arange(B)
        self.lin = np.random.default_rng(5).random((2 * B, 128)) < 0.5       # MLP dropout keep mask, one row per LINK
        self.L = 4
        self.ref = PC.make_ref_model(self.L, case.R, seed=3, adj_dropout=0.0)
        self.flat = None
        self._h0 = {}
        self.geometry = None      # what igmc_model_step_geometry reported (asserted in every run)

    def arena(self):
        return engine.Batch(self.g, max_graphs=self.case.B, hop=1, max_nodes_per_hop=self.case.mnph)

    def workspace(self, b):
        ws = engine.ModelWorkspace(self.be.lib, self.be.device, self.case.R, 4, self.L, 0, b.node_capacity, b.edge_capacity,
                                   b.max_graphs)
        if self.flat is None:
            self.flat = PC.flatten_params(ws, self.ref)
        return ws

    def pair(self):
        b = self.arena()
        return b, self.workspace(b)

    def h0(self, drop):
        """H0: the target batch on a new arena and a new workspace (computed once per mask form, shared, never changed)."""
        if drop not in self._h0:
            res = run_step(self, *self.pair(), self.target, drop)
            assert_finite(res, 'H0')
            self._h0[drop] = res
        return self._h0[drop]

    def params(self, poison=False):
        f = self.flat.copy()
        if poison:
            f[::7] = np.nan
        return self.be.dev(f)

    def assert_geometry(self, ws, b):
        """The family (and the split within it) the case set out to hit -- before anything else: an arena one slot wider
        silently takes other kernels."""
        geo = ws.step_geometry(b, self.case.B)
        for k, v in self.case.expect.items():
            if k == 'loop':
                assert geo['grid'] < self.case.B, geo
            else:
                assert geo[k] == v, (self.case.id, k, geo)
        self.geometry = geo
        return geo


def edge_flags_by_id(d, p=0.2, seed=77):
    """Injected edge-dropout flags of a downloaded batch, a function of the edge's GLOBAL user / item ids and direction
    only -- a subgraph keeps its mask wherever it sits in a batch.  Entry of the dst-sorted CSR: bit 0 = keep(src -> dst),
    bit 1 = keep(dst -> src)."""
    N = d['N']
    dst = np.repeat(np.arange(N, dtype=np.int64), np.diff(d['row_ptr']).astype(np.int64))
    src = d['col'].astype(np.int64)
    row_user = d['node_label'][dst] % 2 == 0
    gd, gs = d['node_gid'][dst].astype(np.uint64), d['node_gid'][src].astype(np.uint64)
    u, v = np.where(row_user, gd, gs), np.where(row_user, gs, gd)
    into_user = row_user.astype(np.uint64)        # direction of src -> dst: 1 = item -> user

    def keep(direction):
        with np.errstate(over='ignore'):
            x = (u << np.uint64(34)) ^ (v << np.uint64(2)) ^ direction ^ np.uint64(seed * 0x9E3779B97F4A7C15 & (2 ** 64 - 1))
            x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            x = x ^ (x >> np.uint64(31))
        return ((x >> np.uint64(40)).astype(np.float64) / float(1 << 24) >= p).astype(np.uint8)
    return keep(into_user) | (keep(np.uint64(1) - into_user) << 1)


def _out_buf(be, B):
    return be.dev(np.concatenate([np.zeros(B, np.float32), np.full(OUT_PAD, np.nan, np.float32)]))


def _outputs(o, B, what):
    assert np.isnan(o[B:]).all(), '%s: an output beyond the batch was written' % what
    assert np.isfinite(o[:B]).all(), '%s: non-finite outputs' % what
    return o[:B]


def _load(cr, b, ws, order, drop, exact_flags=True):
    """Extract links ``order`` into ``b``; injected edge flags when ``drop`` (by id, or -- a batch nobody compares -- drawn by
    the arena's own kernel).  -> (downloaded batch or None, device lin mask)."""
    be, B = cr.be, cr.case.B
    order = np.asarray(order)
    assert len(order) == B
    idx = be.dev(order.astype(np.int32))
    b.extract(be.ptr(cr.lu), be.ptr(cr.lv), be.ptr(cr.ly), be.ptr(idx), 0, B)
    be.sync()
    cr.assert_geometry(ws, b)
    d = None
    if exact_flags:
        d = b.download()
        assert d['B'] == B
        want = [(cr.blocks[i][0], cr.blocks[i][1]) for i in order]
        got = [(int(nu), int(n1 - n0 - nu)) for nu, n0, n1 in zip(d['n_users'], d['node_off'][:-1], d['node_off'][1:])]
        assert got == want, 'the extraction did not give the crafted extents'
        if drop:
            b.set_edge_flags(edge_flags_by_id(d))
    elif drop:
        b.edge_dropout(0.2, False, seed=9, step=1)
    return d, be.dev(cr.lin[order].astype(np.uint8).reshape(-1))


def run_step(cr, b, ws, order, drop, P=None, exact_flags=True):
    """Eval forward, then loss + gradient with injected masks, of links ``order`` on (arena, workspace)."""
    be, B = cr.be, cr.case.B
    P = cr.params() if P is None else P
    d, LM = _load(cr, b, ws, order, drop, exact_flags)
    ev, out = _out_buf(be, B), _out_buf(be, B)
    grad, loss = be.dev(np.zeros(ws.n_params, np.float32)), be.dev(np.zeros(2, np.float32))
    ws.forward(be.ptr(P), b, be.ptr(ev), training=False)
    ws.loss_grad(be.ptr(P), b, be.ptr(out), be.ptr(grad), be.ptr(loss), use_edge_flags=drop, lin_mask=be.ptr(LM), ARR=ARR)
    be.sync()
    return dict(ev=be.host(ev), out=be.host(out), grad=be.host(grad), loss=be.host(loss), d=d, ws=ws, order=np.asarray(order))


class TrainBufs(object):
    def __init__(self, cr, ws):
        be, n = cr.be, ws.n_params
        self.start = cr.flat
        self.P, self.G = be.dev(cr.flat.copy()), be.dev(np.zeros(n, np.float32))
        self.M1, self.M2 = be.dev(np.zeros(n, np.float32)), be.dev(np.zeros(n, np.float32))
        self.loss, self.total = be.dev(np.zeros(2, np.float32)), be.dev(np.zeros(1, np.float64))

    def restore(self, be):
        """The caller overwrites the SAME buffers in place with the start values -- and tells the library nothing."""
        _assign(be, self.P, self.start)
        for buf in (self.G, self.M1, self.M2, self.loss, self.total):
            _assign(be, buf, np.zeros(buf.shape, np.float32 if buf is not self.total else np.float64))


def run_train_step(cr, b, ws, bufs, order, drop, exact_flags=True):
    """``igmc_train_step`` (forward, loss, backward, Adam in the step's own launches) of links ``order``."""
    be, B = cr.be, cr.case.B
    d, LM = _load(cr, b, ws, order, drop, exact_flags)
    out = _out_buf(be, B)
    p = lambda x: engine._p(be.ptr(x))
    be.lib.call('igmc_train_step', ws.handle, p(bufs.P), b.handle, int(drop), p(LM), 0, 0, 1.0, ARR, p(out), p(bufs.G),
                p(bufs.M1), p(bufs.M2), p(bufs.loss), p(bufs.total), None, 1, LR, 0.9, 0.999, 1e-8, 0.0, None)
    be.sync()
    be.lib.call('igmc_model_check', ws.handle, None)
    return dict(out=be.host(out), loss=be.host(bufs.loss), params=be.host(bufs.P), m1=be.host(bufs.M1), m2=be.host(bufs.M2))


# ====================================================================== assertions
def assert_finite(res, what):
    B = len(res['order'])
    _outputs(res['ev'], B, what + ' (eval)')
    _outputs(res['out'], B, what + ' (train)')
    assert np.isfinite(res['loss']).all(), '%s: non-finite loss' % what
    assert np.isfinite(res['grad']).all(), '%s: %d non-finite gradient entries' % (what, int((~np.isfinite(res['grad'])).sum()))


def assert_same(a, b, what, keys=('ev', 'out', 'loss', 'grad')):
    """Value equality (``np.array_equal``: a signed zero is not a finding; the NaN sentinels are compared apart)."""
    for k in keys:
        x, y = a[k], b[k]
        if k in ('ev', 'out'):
            n = len(x) - OUT_PAD
            assert np.isnan(x[n:]).all() and np.isnan(y[n:]).all(), '%s: an output beyond the batch was written' % what
            x, y = x[:n], y[:n]
        assert np.isfinite(x).all() and np.isfinite(y).all(), '%s: non-finite %s' % (what, k)
        if not np.array_equal(x, y):
            bad = np.flatnonzero(x != y)
            raise AssertionError('%s: %s differs at %d of %d entries (first %s; largest difference %.3e)' % (
                what, k, len(bad), x.size, bad[:8].tolist(), float(np.abs(x.astype(np.float64) - y).max())))


def same_batch(d0, d1):
    for k in ('node_off', 'n_users', 'node_label', 'node_gid', 'row_ptr', 'col', 'erel', 'eflag', 'y'):
        assert np.array_equal(d0[k], d1[k]), 'the extracted batch differs with the arena\'s history: %s' % k


def check_histories(cr, drop, with_sides=False):
    """H0 (new arena, new workspace) against H1 (dirty batch first, on the same arena and workspace); ``with_sides``: H2 (dirty
    arena, new workspace) and H3 (new arena, dirty workspace), which say which side leaked.  -> (H0, H1)."""
    h0 = cr.h0(drop)
    b1, ws1 = cr.pair()
    run_step(cr, b1, ws1, cr.dirty, drop, exact_flags=False)
    h1 = run_step(cr, b1, ws1, cr.target, drop)
    same_batch(h0['d'], h1['d'])
    failures = []
    for name, res in [('H1 (dirty arena and workspace)', h1)] + (_side_histories(cr, b1, ws1, drop) if with_sides else []):
        try:
            assert_same(h0, res, name + ' vs H0')
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, '\n'.join(failures)
    return h0, h1


def _side_histories(cr, b1, ws1, drop):
    run_step(cr, b1, ws1, cr.dirty, drop, exact_flags=False)          # arena and workspace dirty again
    h2 = run_step(cr, b1, cr.workspace(b1), cr.target, drop)          # dirty arena, new workspace
    b3 = cr.arena()
    h3 = run_step(cr, b3, ws1, cr.target, drop)                       # new arena, dirty workspace
    return [('H2 (dirty arena, new workspace)', h2), ('H3 (new arena, dirty workspace)', h3)]


def check_train_step_history(cr, drop):
    """HT: ``igmc_train_step`` on the dirty batch; the caller then overwrites the same parameter, moment and gradient buffers
    in place with the start values (no ``igmc_model_weights_unchanged``); ``igmc_train_step`` on the target.  Parameters, both
    Adam moments, loss and outputs equal those of a train step on new memory -- stale weight images behind an in-place
    parameter change included."""
    be = cr.be
    b0, ws0 = cr.pair()
    t0 = run_train_step(cr, b0, ws0, TrainBufs(cr, ws0), cr.target, drop)
    b, ws = cr.pair()
    bufs = TrainBufs(cr, ws)
    run_train_step(cr, b, ws, bufs, cr.dirty, drop, exact_flags=False)
    bufs.restore(be)
    be.sync()
    t1 = run_train_step(cr, b, ws, bufs, cr.target, drop)
    assert not np.array_equal(t0['params'], cr.flat), 'the step did not move the parameters'
    assert_same(t0, t1, 'HT (train step after a dirty train step) vs a train step on new memory',
                keys=('out', 'loss', 'params', 'm1', 'm2'))
    return t0


def check_positions(cr, drop, both_halves=True):
    """Each subgraph's eval and training outputs are the same values wherever it sits: under a permuted link order
    (``link_idx``, the mask rows permuted alike) and interleaved with dirty blocks as batch-mates.  (Gradients are ordered
    sums over the batch: not asserted here.)"""
    B, h0 = cr.case.B, cr.h0(drop)
    perm = np.random.default_rng(11).permutation(B)
    if B > 1 and np.array_equal(perm, np.arange(B)):
        perm = np.roll(perm, 1)
    runs = [('permuted', cr.target[perm], np.arange(B), perm)]
    h = (B + 1) // 2
    a = np.array([cr.target[k // 2] if k % 2 == 0 else cr.dirty[k] for k in range(B)])
    runs.append(('dirty batch-mates (even slots)', a, np.arange(0, B, 2), np.arange(h)))
    if B > 1 and both_halves:
        c = np.array([cr.dirty[k] if k % 2 == 0 else cr.target[h + k // 2] for k in range(B)])
        runs.append(('dirty batch-mates (odd slots)', c, np.arange(1, B, 2), h + np.arange(B // 2)))
    for name, order, where, which in runs:
        res = run_step(cr, *cr.pair(), order, drop)
        assert_finite(res, name)
        for k in ('ev', 'out'):
            got, want = res[k][where], h0[k][which]
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError('%s: %s of target subgraphs %s (extents %s) depend on their position' % (
                    name, k, which[bad][:8].tolist(), [cr.case.targets[i] for i in which[bad][:8]]))


def check_oracle(cr, res, drop):
    """A result against ``oracle/pyg_ref`` in float64 on the identical batch, weights and masks, at the suite's parity
    tolerances; the float32 oracle's own distance from float64 is recorded beside the engine's."""
    import torch
    from oracle import pyg_ref
    d, B = res['d'], len(res['order'])
    edge_mask = torch.from_numpy((edge_flags_by_id(d) & 1).astype(bool)) if drop else None
    lin_mask = torch.from_numpy(cr.lin[res['order']])
    got = {}
    for dt in (torch.float64, torch.float32):
        m = PC.make_ref_model(cr.L, cr.case.R, seed=3, adj_dropout=0.2 if drop else 0.0).to(dt)
        pyg = batch_to_pyg(d, cr.L)
        pyg.x, pyg.y = pyg.x.to(dt), pyg.y.to(dt)
        _, ev = pyg_ref.eval_sse(m, pyg)
        rl, ro, rg = pyg_ref.loss_and_grads(m, pyg, ARR=ARR, edge_mask=edge_mask, lin_mask=lin_mask)
        got[dt] = (ev.numpy().astype(np.float64), ro.numpy().astype(np.float64), float(rl),
                   {k: v.numpy().astype(np.float64) for k, v in rg.items()})
    ev64, out64, loss64, g64 = got[torch.float64]

    def errors(ev, out, loss, grads):
        worst, key = 0.0, ''
        for k, r in g64.items():
            e = float(np.abs(grads[k] - r).max() / max(np.abs(r).max(), 1e-6))
            if e > worst:
                worst, key = e, k
        return dict(eval_out_rel=PC.rel_err(ev, ev64), train_out_rel=PC.rel_err(out, out64),
                    loss_rel=abs(loss - loss64) / max(abs(loss64), 1e-12), worst_grad_rel=worst, worst_grad_tensor=key)
    eng = errors(res['ev'][:B], res['out'][:B], float(res['loss'][0]), PC.unflatten_grads(res['ws'], res['grad']))
    f32 = errors(*got[torch.float32])
    PC.record_observed('history_parity', case=cr.case.id, backend=cr.be.name, B=int(B), N=int(d['N']), E=int(d['E']),
                       dropout=bool(drop), **dict(list(eng.items()) + [('f32_oracle_' + k, v) for k, v in f32.items()]))
    assert eng['eval_out_rel'] < PC.OUT_TOL and eng['train_out_rel'] < PC.OUT_TOL, (eng, f32)
    assert eng['loss_rel'] < PC.LOSS_RTOL, (eng, f32)
    assert eng['worst_grad_rel'] < PC.GRAD_TOL, (eng, f32)
    return eng, f32


def run_nonfinite_history(cr, drop=False):
    """The dirty batch on parameters in which every 7th value is NaN (eval forward + loss / gradient, no Adam), then
    ``igmc_model_reset_exchange``, then the target on the good parameters: equal to the target on new memory.  (Without the
    reset a NaN row left in a slot's exchange region meets the zero block bytes of a smaller subgraph: 0 * NaN.)"""
    be = cr.be
    h0 = cr.h0(drop)
    b, ws = cr.pair()
    bad = run_step(cr, b, ws, cr.dirty, drop, P=cr.params(poison=True), exact_flags=False)
    assert not np.isfinite(bad['out'][:cr.case.B]).any(), 'the poisoned parameters did not reach the outputs'
    be.lib.call('igmc_model_reset_exchange', ws.handle, None)
    res = run_step(cr, b, ws, cr.target, drop)
    assert_same(h0, res, 'target after a step on non-finite parameters and igmc_model_reset_exchange vs H0')
    return h0
