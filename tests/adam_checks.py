"""One optimiser step of every Adam tail against float64 Adam, element by element -- shared by tests/test_emu_adam_tails.py
(host emulation of the HIP sources) and tests/test_gpu_adam_tails.py (the gfx950 library).

Every fused tail stores the flat gradient it used (``grad[i] = g`` in ``fts_emit``, before weight decay), so the optimiser can be
separated from the gradient's float noise: with ``P0, M1_0, M2_0`` known and ``G, P1, M1_1, M2_1`` read back, each element of
the step is one short chain of float32 operations, held here to its float64 value within a COUNT of roundings
(``eps = 2^-24``; no chain has more than 6 / 9 / 8 roundings, division and square root are correctly rounded -- the build
passes no fast-math flag -- and contraction into an fma only removes roundings):

    M1_1 = b1 M1_0 + (1 - b1) gi            gi = G + wd P0      |error| <= 8 eps (|b1 M1_0| + (1 - b1)(|G| + |wd P0|))
    M2_1 = b2 M2_0 + (1 - b2) gi^2                              |error| <= 12 eps (|b2 M2_0| + (1 - b2)(|G| + |wd P0|)^2)
    P1   = P0 - u,   u = lr / (1 - b1^t) M1_1 / (sqrt(M2_1) / sqrt(1 - b2^t) + eps_adam)    (from the STORED moments)
                                                                |error| <= eps |P1| + 10 eps |u|

No element is exempt.  The hyper-parameters are the float32 values the kernels receive on either route (arguments; the control
block's doubles, which the kernels narrow to float).  The gradient itself is held to ``oracle/pyg_ref`` in float64 at the
suite's parity tolerances, the loss likewise: identity + gradient = the whole step.

The moments a step starts from are NOT zero (``start_moments``), the step number is not 1 and the hyper-parameters are not the
defaults (H1: weight decay, another eps, other betas) -- where a tail that re-forms a neighbour's parameter from stashed
moments, or reads a scalar from the wrong place, goes wrong."""
import ctypes as C

import numpy as np

import parity_checks as PC
from helpers import batch_to_pyg, random_rating_graph
from igmc_amd import _lib, engine
from igmc_amd.stepgraph import _ctrl_words

EPS32 = 2.0 ** -24
ARR = 0.001
H0 = (1e-3, 0.9, 0.999, 1e-8, 0.0)           # the project's defaults: lr, beta1, beta2, eps, weight_decay
H1 = (3e-3, 0.8, 0.95, 1e-6, 0.01)
T_STEPS = (1, 7, 100000)                     # beta2^t: ~e^-100 for H0's beta2 at the last, underflows for H1's
HOOKS = ('IGMC_GRAPH_STEP', 'IGMC_GS_CLUSTER', 'IGMC_GS_GRID', 'IGMC_DL', 'IGMC_DL_ALWAYS', 'IGMC_DL_FUSED', 'IGMC_DL_TS',
         'IGMC_DL_GSPLIT', 'IGMC_DL_HEAD', 'IGMC_FIN_MODE', 'IGMC_TAIL_FOLD')
STEP0 = 11                                   # the control block's step counter at the first step (any value)


def as_f32(h):
    """The hyper-parameters as a kernel holds them: float32, returned as Python floats (exact)."""
    return tuple(float(np.float32(x)) for x in h)


def start_moments(n, seed=17):
    """M1_0 = 1e-3 N(0,1), M2_0 = (1e-3 N(0,1))^2; every 13th element of M2_0 is 1e4, every 11th of both exactly 0."""
    rng = np.random.default_rng(seed)
    m1 = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    m2 = ((1e-3 * rng.standard_normal(n)) ** 2).astype(np.float32)
    m2[::13] = 1e4
    m1[::11] = 0.0
    m2[::11] = 0.0
    return m1, m2


def adam_identity(P0, M1_0, M2_0, G, P1, M1_1, M2_1, t, hyp, what=''):
    """The three rows of the identity on every element.  -> worst element of each row in units of its bound."""
    lr, b1, b2, eps, wd = [np.float64(x) for x in as_f32(hyp)]
    for name, a in (('G', G), ('P1', P1), ('M1_1', M1_1), ('M2_1', M2_1)):
        assert np.isfinite(a).all(), '%s: non-finite %s' % (what, name)
    P0, M1_0, M2_0, G = [np.asarray(a, np.float64) for a in (P0, M1_0, M2_0, G)]
    P1, M1_1, M2_1 = [np.asarray(a, np.float64) for a in (P1, M1_1, M2_1)]
    gi = G + wd * P0
    ga = np.abs(G) + np.abs(wd * P0)
    rows = []
    rows.append(('exp_avg', M1_1, b1 * M1_0 + (1 - b1) * gi, 8 * EPS32 * (np.abs(b1 * M1_0) + (1 - b1) * ga)))
    rows.append(('exp_avg_sq', M2_1, b2 * M2_0 + (1 - b2) * gi * gi, 12 * EPS32 * (np.abs(b2 * M2_0) + (1 - b2) * ga * ga)))
    tt = np.float64(t)
    u = lr / (1.0 - b1 ** tt) * M1_1 / (np.sqrt(M2_1) / np.sqrt(1.0 - b2 ** tt) + eps)
    rows.append(('param', P1, P0 - u, EPS32 * np.abs(P1) + 10 * EPS32 * np.abs(u)))
    worst = {}
    for name, got, ref, bound in rows:
        err = np.abs(got - ref)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        i = int(np.argmax(ratio))
        worst[name] = float(ratio[i])
        assert ratio[i] <= 1.0, ('%s: %s of element %d is %.9g, float64 Adam gives %.9g: %.2f of the bound (%d of %d elements '
                                 'over it); t = %d, hyper-parameters %s' % (what, name, i, got[i], ref[i], ratio[i],
                                                                            int((ratio > 1.0).sum()), len(ratio), t, (hyp,)))
    assert np.abs(u).max() > 0, '%s: the step moved nothing' % what
    return worst


def ctrl_doubles(w):
    return np.asarray(w, np.int64).view(np.float64)


def check_ctrl_advanced(w, t_next, hyp_in_block, what=''):
    """After a step's tick: ADAM_T is ``t_next`` and the two derived doubles are those of ``t_next`` (device pow within 2 ulp,
    subtracted from a correction of at least 1 - beta2 = 1e-3: 1e-12 relative is generous by three orders)."""
    lr, b1, b2 = [float(x) for x in hyp_in_block[:3]]
    assert int(w[_lib.CTRL['ADAM_T']]) == t_next, (what, int(w[_lib.CTRL['ADAM_T']]), t_next)
    d = ctrl_doubles(w)
    want_ss = lr / (1.0 - b1 ** t_next)
    want_bc = 1.0 / np.sqrt(1.0 - b2 ** t_next)
    assert abs(d[_lib.CTRL['STEP_SIZE']] - want_ss) <= 1e-12 * want_ss, (what, d[_lib.CTRL['STEP_SIZE']], want_ss)
    assert abs(d[_lib.CTRL['INV_SQRT_BC2']] - want_bc) <= 1e-12 * want_bc, (what, d[_lib.CTRL['INV_SQRT_BC2']], want_bc)
    assert d[_lib.CTRL['LR']] == lr, (what, d[_lib.CTRL['LR']], lr)
    assert int(w[_lib.CTRL['SYNC_ERR']]) == 0, (what, int(w[_lib.CTRL['SYNC_ERR']]))


def set_lr_like_begin_epoch(w, lr, t):
    """The LR word and STEP_SIZE of a new learning rate, as ``StepGraph.begin_epoch`` writes them (``_ctrl_words``)."""
    d = ctrl_doubles(w)
    src = ctrl_doubles(_ctrl_words(0, 0, t, 1, 1, lr, d[_lib.CTRL['BETA1']], d[_lib.CTRL['BETA2']], d[_lib.CTRL['EPS']],
                                   d[_lib.CTRL['WD']]))
    for k in ('LR', 'STEP_SIZE', 'INV_SQRT_BC2'):
        d[_lib.CTRL[k]] = src[_lib.CTRL[k]]
    return w


def _assign(be, buf, arr):
    if be.name == 'emu':
        buf[...] = arr
    else:
        buf.copy_(be.torch.from_numpy(np.ascontiguousarray(arr)))


def weight_images(be, ws):
    fn = be.lib.cdll.igmc_debug_weight_images
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    n = C.c_int64(0)
    be.sync()
    assert fn(ws.handle, None, C.byref(n)) == 0 and n.value > 0
    out = np.zeros(n.value, np.uint32)
    assert fn(ws.handle, C.c_void_p(out.ctypes.data), C.byref(n)) == 0
    return out


# ====================================================================== the rows: one per form of the tail
class Row(object):
    def __init__(self, id, R=5, hooks=(), how='train_step', expect=(), ran=(), not_ran=(), cap=12):
        self.id, self.R, self.hooks, self.how, self.cap = id, R, dict(hooks), how, cap
        self.expect, self.ran, self.not_ran = dict(expect), tuple(ran), tuple(not_ran)


def _sub(cs):
    return dict(IGMC_GRAPH_STEP='1', IGMC_GS_CLUSTER=str(cs))


_DENSE = dict(IGMC_DL_ALWAYS='1', IGMC_GRAPH_STEP='0')
ROWS = {}
for _cs in (1, 2, 4):
    # the subgraph kernel + the one-launch tail (the default), one workgroup / clusters of 2 and 4 per subgraph
    ROWS['fold_cs%d' % _cs] = Row('fold_cs%d' % _cs, hooks=_sub(_cs), expect=dict(family='subgraph', wg_per_graph=_cs, tables=1),
                                  ran=('k_graph_step', 'k_tail_fin'), not_ran=('k_tail_ts', 'k_finalize_adam', 'k_adam'))
    # ... + the two-launch tail
    ROWS['ts_cs%d' % _cs] = Row('ts_cs%d' % _cs, hooks=dict(_sub(_cs), IGMC_TAIL_FOLD='0'),
                                expect=dict(family='subgraph', wg_per_graph=_cs, tables=1),
                                ran=('k_graph_step', 'k_tail_ts', 'k_finalize_adam'), not_ran=('k_tail_fin', 'k_adam'))
ROWS['dense_r5'] = Row('dense_r5', hooks=_DENSE, expect=dict(groups=1, tables=1), ran=('k_tail_ts', 'k_finalize_adam'),
                       not_ran=('k_graph_step', 'k_tail_fin', 'k_reduce_partials', 'k_adam'))
# two relation groups: the tables' tail takes its columns through the R > 8 body
ROWS['dense_r10'] = Row('dense_r10', R=10, hooks=dict(IGMC_DL_ALWAYS='1'), expect=dict(family='dense_fused', groups=2, tables=1),
                        ran=('k_tail_ts', 'k_finalize_adam'), not_ran=('k_graph_step', 'k_tail_fin', 'k_reduce_partials', 'k_adam'))
# row walkers: k_reduce_partials -> k_finalize_ts in basis-space mode
ROWS['rows_bs'] = Row('rows_bs', hooks=dict(IGMC_GRAPH_STEP='0', IGMC_DL='0'), expect=dict(family='rows', tables=0),
                      ran=('k_reduce_partials', 'k_finalize_adam'), not_ran=('k_graph_step', 'k_tail_ts', 'k_tail_fin', 'k_adam'))
# the hand-off tail k_finalize with its AdamTail: no stash, so neither the one-launch tail (asked for by default) nor
# k_finalize_ts can run -- k_tail_ts sums the tables, 'k_finalize_adam' is k_finalize
ROWS['handoff'] = Row('handoff', hooks=dict(_sub(1), IGMC_FIN_MODE='0'), expect=dict(family='subgraph', wg_per_graph=1),
                      ran=('k_graph_step', 'k_tail_ts', 'k_finalize_adam'), not_ran=('k_tail_fin', 'k_adam'))
# the ragged-batch sequence of StepGraph._model / _finish
ROWS['finish'] = Row('finish', hooks=_sub(1), how='finish', expect=dict(family='subgraph'),
                     ran=('k_graph_step', 'k_finalize', 'k_step_finish'), not_ran=('k_finalize_adam', 'k_tail_fin', 'k_adam'))
ROWS['dp'] = Row('dp', hooks=_sub(1), how='dp', expect=dict(family='subgraph', wg_per_graph=1, tables=1),
                 ran=('k_graph_step', 'k_tail_fin'), not_ran=('k_tail_ts', 'k_finalize_adam', 'k_adam'))
ROWS['sortpool'] = Row('sortpool', hooks=(), how='sortpool', ran=('k_step_finish',), not_ran=('k_finalize_adam', 'k_tail_fin', 'k_adam'))


# (row, B, edge dropout, hyper-parameters, Adam steps of the argument route, first Adam step of the control-block route)
CASES = [
    ('fold_cs1', 7, True, H1, (1, 100000), 7),
    ('fold_cs2', 7, False, H1, (7,), 1),
    ('fold_cs4', 17, True, H1, (7,), 100000),
    ('fold_cs1', 7, False, H0, (1, 7, 100000), 1),
    ('ts_cs1', 7, False, H1, (1, 100000), 7),
    ('ts_cs2', 7, True, H1, (7,), 100000),
    ('ts_cs4', 17, False, H1, (7,), 1),
    ('dense_r5', 7, True, H1, (1, 7, 100000), 7),
    ('dense_r5', 7, False, H0, (7,), 100000),
    ('dense_r10', 7, True, H1, (1, 7, 100000), 7),
    ('rows_bs', 7, True, H1, (1, 7, 100000), 7),
    ('handoff', 7, True, H1, (1, 7, 100000), 7),
    ('finish', 7, True, H1, (1, 7, 100000), 7),
    ('finish', 7, False, H0, (7,), 1),
    ('sortpool', 7, True, H1, (1, 7, 100000), 7),
    ('dp', 7, True, H1, (1, 7, 100000), 7),
]
IDS = ['%s-B%d-%s-%s' % (r, B, 'drop' if d else 'nodrop', 'H0' if h == H0 else 'H1') for r, B, d, h, _, _ in CASES]


def set_hooks(monkeypatch, row):
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    for k, v in row.hooks.items():
        monkeypatch.setenv(k, v)


_DATA = {}


def links_of(R):
    """The small graph of test_emu_tail_fold.py (its rated pairs as links, twice permuted)."""
    if R not in _DATA:
        A = random_rating_graph(44, 40, 0.3, R, seed=20)
        rows, cols = A.nonzero()
        lu, lv = rows.astype(np.int32).copy(), cols.astype(np.int32).copy()
        ly = np.asarray(A[rows, cols]).ravel().astype(np.float32)
        rng = np.random.default_rng(3)
        perm = np.concatenate([rng.permutation(len(lu)) for _ in range(2)]).astype(np.int32)
        _DATA[R] = (A, lu, lv, ly, perm)
    return _DATA[R]


def edge_flags(d, seed):
    """Injected keep flags of a downloaded batch: bit 0 = keep(src -> dst), bit 1 = keep(dst -> src)."""
    keep = np.random.default_rng(seed).random(d['E']) >= 0.2
    rev = PC.reverse_positions(d)
    return keep, keep.astype(np.uint8) | (keep[rev].astype(np.uint8) << 1)


class Fused(object):
    """Arena, workspace and device buffers of one row at batch size B; ``step`` runs one optimiser step of the row's form from
    given parameters, moments, step number and scalars and checks all of it."""

    def __init__(self, be, monkeypatch, row, B, drop):
        import torch
        from oracle import pyg_ref
        self.be, self.row, self.B, self.drop = be, row, B, drop
        set_hooks(monkeypatch, row)
        lib = be.lib
        A, lu, lv, ly, perm = links_of(row.R)
        assert len(perm) >= 4 * B
        self.g = engine.Graph(A, device=be.device, lib=lib)
        self.links = [be.dev(a) for a in (lu, lv, ly, perm)]
        self.batch = engine.Batch(self.g, B, 1, 16 if B > 7 else row.cap)      # (per-hop caps: 12, and 16 under the batches of 17)
        b = self.batch
        self.ws = engine.ModelWorkspace(lib, be.device, row.R, 4, 4, 0, b.node_capacity, b.edge_capacity, B)
        self.sp = None
        if row.how == 'sortpool':
            self.sp = engine.SortPoolWorkspace(self.ws, 12, max(2, b.node_capacity // b.max_graphs))
            torch.manual_seed(4)
            self.ref = pyg_ref.DGCNNRSRef(4, (32, 32, 32, 1), 12, row.R, 4, adj_dropout=0.2 if drop else 0.0, fast=True)
            with torch.no_grad():
                for p in self.ref.parameters():
                    p.add_(0.05 * torch.randn_like(p))
            self.n = self.sp.n_params
            self.spans = [(k, off, tuple(self.ref.state_dict()[k].shape)) for k, off in self.sp.offsets.items()]
            assert sum(int(np.prod(s)) for _, _, s in self.spans) == self.n
        else:
            self.ref = PC.make_ref_model(4, row.R, seed=4, adj_dropout=0.2 if drop else 0.0)
            self.n = self.ws.n_params
            self.spans = list(self.ws.layout())
        sd = {k: v.detach().numpy().astype(np.float32) for k, v in self.ref.state_dict().items()}
        self.P0 = np.zeros(self.n, np.float32)
        for k, off, shape in self.spans:
            self.P0[off:off + int(np.prod(shape))] = sd[k].reshape(-1)
        self.ref = self.ref.double()
        self.M1_0, self.M2_0 = start_moments(self.n)
        z = lambda m, dt=np.float32: be.dev(np.zeros(m, dt))
        self.P, self.M1, self.M2, self.G = z(self.n), z(self.n), z(self.n), z(self.n)
        self.loss, self.total = z(2), z(1, np.float64)
        self.ctrl = be.dev(np.zeros(_lib.CTRL['WORDS'], np.int64))
        self.lin = np.random.default_rng(5).random((4, B, 128)) < 0.5
        self.attached = False
        self.k = 0            # steps since the control block was written: which batch the selector resolves

    def close(self):
        if self.attached:
            self.attach(False)

    def attach(self, on):
        cp = engine._p(self.be.ptr(self.ctrl)) if on else None
        self.be.lib.call('igmc_batch_set_ctrl', self.batch.handle, cp)
        self.be.lib.call('igmc_model_set_ctrl', self.ws.handle, cp)
        self.attached = on

    def load_state(self, P=None, M1=None, M2=None):
        be = self.be
        _assign(be, self.P, self.P0 if P is None else P)
        _assign(be, self.M1, self.M1_0 if M1 is None else M1)
        _assign(be, self.M2, self.M2_0 if M2 is None else M2)
        _assign(be, self.G, np.zeros(self.n, np.float32))

    def write_ctrl(self, t, hyp):
        """The control block of Adam step ``t`` with ``hyp`` (float32 values, as doubles).
        (float32 VALUES on purpose: the kernels narrow the block's betas to float for the moments, but ``_ctrl_words`` and
        ``ctrl_advance`` form the two bias corrections from the block's doubles, while ``adam_scalars`` -- the argument route --
        forms them from the narrowed floats.  With beta2 = 0.999 as a double the two routes' 1 / sqrt(1 - beta2^t) differ by
        6e-6 relative at t = 1 (500 x the float rounding of 0.999), less with every step; torch forms them in double, as the
        block does.  Writing float32 values makes the two routes one reference.)"""
        w = _ctrl_words(STEP0, 0, t, self.B, 1, *as_f32(hyp))
        _assign(self.be, self.ctrl, w)
        self.k = 0
        if not self.attached:
            self.attach(True)

    def _oracle(self, P_now, d, lm, keep):
        """loss and gradients of ``oracle/pyg_ref`` in float64 on the identical batch, parameters and masks."""
        import torch
        from oracle import pyg_ref
        with torch.no_grad():
            sd = self.ref.state_dict()
            for k, off, shape in self.spans:
                sd[k].copy_(torch.from_numpy(P_now[off:off + int(np.prod(shape))].astype(np.float64).reshape(shape)))
        pyg = batch_to_pyg(d, 4)
        pyg.x, pyg.y = pyg.x.double(), pyg.y.double()
        em = torch.from_numpy(keep) if keep is not None else None
        if self.sp is None:
            rl, ro, rg = pyg_ref.loss_and_grads(self.ref, pyg, ARR=ARR, edge_mask=em, lin_mask=torch.from_numpy(lm))
            return float(rl), ro.numpy(), {k: v.numpy() for k, v in rg.items()}
        self.ref.train()
        self.ref.zero_grad()
        to = self.ref(pyg, edge_mask=em, lin_mask=torch.from_numpy(lm))
        rl = PC.F_mse(to, pyg.y) + ARR * pyg_ref.arr_loss(self.ref)
        rl.backward()
        return float(rl.detach()), to.detach().numpy(), {k: p.grad.detach().numpy() for k, p in self.ref.named_parameters()}

    def step(self, t, hyp, route, hyp_args=None, what=''):
        """One step at Adam step ``t``.  ``route`` 'args': the scalars as arguments, no control block; 'ctrl': from the control
        block as it stands (``write_ctrl`` / the previous step's tick), the arguments carrying ``hyp_args`` -- which the step
        must ignore.  -> dict(worst=..., P1, M1_1, M2_1, G, out, loss, ctrl)"""
        be, row, B, lib = self.be, self.row, self.B, self.be.lib
        p = lambda x: engine._p(be.ptr(x))
        lu, lv, ly, perm = self.links
        use_ctrl = route == 'ctrl'
        if use_ctrl:
            assert self.attached
            self.batch.extract(be.ptr(lu), be.ptr(lv), be.ptr(ly), be.ptr(perm), self.k & 1, B, 1.0, 7, 999)
        else:
            if self.attached:
                self.attach(False)
            self.batch.extract(be.ptr(lu), be.ptr(lv), be.ptr(ly), be.ptr(perm), 0, B, 1.0, 7, 3)
        be.sync()
        # the form, before any number is looked at
        geo = self.ws.step_geometry(self.batch, B)
        for k, v in row.expect.items():
            assert geo[k] == v, (row.id, k, geo)
        if row.id.startswith('dense'):
            assert geo['family'] in ('dense_fused', 'dense_layer'), geo
            assert self.batch.dense_layers(self.ws)
        d = self.batch.download()
        assert d['B'] == B
        keep = None
        if self.drop:
            keep, flags = edge_flags(d, 100 + self.k)
            self.batch.set_edge_flags(flags)
        lm = self.lin[self.k % len(self.lin)]
        LM = be.dev(lm.astype(np.uint8).reshape(-1))
        out = be.dev(np.concatenate([np.zeros(B, np.float32), np.full(8, np.nan, np.float32)]))
        before = [be.host(x).copy() for x in (self.P, self.M1, self.M2)]
        ctrl0 = be.host(self.ctrl).copy()
        a = as_f32(hyp_args if (use_ctrl and hyp_args is not None) else hyp)
        cp = p(self.ctrl) if use_ctrl else None
        t_arg = 1 if use_ctrl else t
        engine.profile_fetch(lib)
        engine.profile_enable(lib, True)
        try:
            if row.how in ('train_step', 'dp'):
                args = (p(self.P), self.batch.handle, int(self.drop), p(LM), 0, 0, 1.0, ARR, p(out), p(self.G), p(self.M1),
                        p(self.M2), p(self.loss), p(self.total), cp, t_arg) + a + (None,)
                if row.how == 'dp':
                    lib.call('igmc_train_step_dp', self.ws.handle, None, *args)
                else:
                    lib.call('igmc_train_step', self.ws.handle, *args)
            else:
                fam = self.ws if self.sp is None else self.sp
                fam.loss_grad(be.ptr(self.P), self.batch, be.ptr(out), be.ptr(self.G), None, use_edge_flags=self.drop,
                              lin_mask=be.ptr(LM), ARR=ARR, grad_scale=1.0 / B)
                fn = 'igmc_step_finish' if self.sp is None else 'igmc_sortpool_step_finish'
                lib.call(fn, fam.handle, self.batch.handle, p(self.P), p(self.G), p(self.M1), p(self.M2), ARR, p(self.loss),
                         p(self.total), cp, t_arg, *(a + (None,)))
            be.sync()
        finally:
            engine.profile_enable(lib, False)
        labels = {n: c for n, _, c in engine.profile_fetch(lib)}
        for name in row.ran:
            assert labels.get(name, 0) >= 1, (row.id, 'did not run', name, labels)
        for name in row.not_ran:
            assert name not in labels, (row.id, 'ran', name, labels)
        lib.call('igmc_model_check', self.ws.handle, None)
        P1, M1_1, M2_1, G = [be.host(x).copy() for x in (self.P, self.M1, self.M2, self.G)]
        o, loss = be.host(out), be.host(self.loss).copy()
        assert np.isnan(o[B:]).all(), '%s: an output beyond the batch was written' % what
        assert np.isfinite(o[:B]).all() and np.isfinite(loss).all(), '%s: non-finite outputs or loss' % what
        # ---- the optimiser, element by element
        worst = adam_identity(before[0], before[1], before[2], G, P1, M1_1, M2_1, t, hyp, what=what)
        # ---- the gradient it used, the outputs and the loss against the oracle in float64
        rl, ro, rg = self._oracle(before[0], d, lm, keep)
        gtol = PC.GRAD_TOL if self.sp is None else PC.DGCNN_GRAD_TOL
        otol = PC.OUT_TOL if self.sp is None else PC.DGCNN_OUT_TOL
        ltol = PC.LOSS_RTOL if self.sp is None else PC.DGCNN_LOSS_RTOL
        gw, gk = 0.0, ''
        for k, off, shape in self.spans:
            if k not in rg:
                continue
            r = rg[k].reshape(-1)
            e = float(np.abs(G[off:off + r.size] - r).max() / max(np.abs(r).max(), 1e-6))
            if e > gw:
                gw, gk = e, k
        worst.update(grad_rel=gw, out_rel=PC.rel_err(o[:B], ro), loss_rel=abs(float(loss[0]) - rl) / max(abs(rl), 1e-12))
        PC.record_observed('adam_identity', row=row.id, backend=be.name, B=int(B), dropout=bool(self.drop), route=route, t=int(t),
                           hyper='H0' if tuple(hyp) == H0 else 'H1' if tuple(hyp) == H1 else str(tuple(hyp)), **worst)
        assert gw < gtol, '%s: %s: max rel-to-peak gradient error %.3e' % (what, gk, gw)
        assert worst['out_rel'] < otol, (what, worst)
        assert worst['loss_rel'] < ltol, (what, worst)
        ctrl1 = be.host(self.ctrl).copy()
        if use_ctrl:
            assert int(ctrl0[_lib.CTRL['ADAM_T']]) == t
            check_ctrl_advanced(ctrl1, t + 1, ctrl_doubles(ctrl0)[[_lib.CTRL['LR'], _lib.CTRL['BETA1'], _lib.CTRL['BETA2']]], what)
            assert int(ctrl1[_lib.CTRL['STEP']]) == int(ctrl0[_lib.CTRL['STEP']]) + 1
            self.k += 1
        else:
            assert np.array_equal(ctrl0, ctrl1)
        return dict(worst=worst, P1=P1, M1_1=M1_1, M2_1=M2_1, G=G, out=o[:B], loss=loss, ctrl=ctrl1, lm=LM, d=d)


def check_step(be, monkeypatch, row, B, drop, hyp, t, route):
    """Section 1 on one row: a step from ``(P0, M1_0, M2_0)`` at Adam step ``t``.  'ctrl': the block carries ``hyp`` and the
    arguments the OTHER set; three consecutive steps, the device's own advance checked after each, and a learning rate
    rewritten between the second and the third the way ``begin_epoch`` does."""
    f = Fused(be, monkeypatch, ROWS[row] if isinstance(row, str) else row, B, drop)
    try:
        f.load_state()
        what = '%s B=%d drop=%d %s t=%d' % (f.row.id, B, drop, route, t)
        if route == 'args':
            return [f.step(t, hyp, 'args', what=what)]
        other = H0 if tuple(hyp) != H0 else H1
        f.write_ctrl(t, hyp)
        res = [f.step(t, hyp, 'ctrl', hyp_args=other, what=what + ' step 1'),
               f.step(t + 1, hyp, 'ctrl', hyp_args=other, what=what + ' step 2')]
        lr2 = float(np.float32(np.float32(hyp[0]) * np.float32(0.1)))
        w = set_lr_like_begin_epoch(be.host(f.ctrl).copy(), lr2, t + 2)
        _assign(be, f.ctrl, w)
        hyp2 = (lr2,) + tuple(hyp[1:])
        res.append(f.step(t + 2, hyp2, 'ctrl', hyp_args=other, what=what + ' step 3 (lr x 0.1)'))
        assert ctrl_doubles(res[-1]['ctrl'])[_lib.CTRL['LR']] == lr2
        return res
    finally:
        f.close()


def check_images(be, monkeypatch, row, B, drop, hyp=H1, t=7):
    """Section 5: the weight images a weight-decayed step leaves are, word for word, the ones a new workspace composes from
    the parameters it left -- and an evaluation forward that rides on them gives that workspace's outputs bit for bit."""
    f = Fused(be, monkeypatch, ROWS[row], B, drop)
    try:
        f.load_state()
        r = f.step(t, hyp, 'args', what='%s images' % row)
        left = weight_images(be, f.ws)
        b = f.batch
        ws2 = engine.ModelWorkspace(be.lib, be.device, f.row.R, 4, 4, 0, b.node_capacity, b.edge_capacity, B)
        P1 = be.dev(r['P1'])
        out2, out1 = be.dev(np.zeros(B, np.float32)), be.dev(np.zeros(B, np.float32))
        ws2.forward(be.ptr(P1), b, be.ptr(out2), training=False)
        composed = weight_images(be, ws2)
        assert left.shape == composed.shape
        bad = np.flatnonzero(left != composed)
        assert not len(bad), '%s: %d of %d image words differ from the composed ones (first %s)' % (row, len(bad), len(left), bad[:8])
        be.lib.call('igmc_model_weights_unchanged', f.ws.handle, 1)
        engine.profile_fetch(be.lib)
        engine.profile_enable(be.lib, True)
        try:
            f.ws.forward(be.ptr(f.P), b, be.ptr(out1), training=False)
            be.sync()
        finally:
            engine.profile_enable(be.lib, False)
        labels = {n: c for n, _, c in engine.profile_fetch(be.lib)}
        assert 'k_g2_compose' not in labels, labels       # the forward read the images the step left
        o1, o2 = be.host(out1), be.host(out2)
        assert np.isfinite(o2).all() and np.array_equal(o1, o2), (o1, o2)
    finally:
        f.close()


def check_flat_adam(be, n, hyp, t, route='args'):
    """``igmc_adam_step`` / ``igmc_adam_step_ctrl`` (k_adam) over n elements with a random gradient."""
    rng = np.random.default_rng(n)
    P0 = rng.standard_normal(n).astype(np.float32)
    G0 = (1e-2 * rng.standard_normal(n)).astype(np.float32)
    G0[3::7] = 0.0
    M1_0, M2_0 = start_moments(n)
    P, G, M1, M2 = be.dev(P0.copy()), be.dev(G0.copy()), be.dev(M1_0.copy()), be.dev(M2_0.copy())
    p = lambda x: engine._p(be.ptr(x))
    engine.profile_fetch(be.lib)
    engine.profile_enable(be.lib, True)
    try:
        if route == 'args':
            be.lib.call('igmc_adam_step', p(P), p(G), p(M1), p(M2), n, t, *(as_f32(hyp) + (None,)))
        else:
            ctrl = be.dev(_ctrl_words(STEP0, 0, t, 1, 1, *as_f32(hyp)))
            be.lib.call('igmc_adam_step_ctrl', p(P), p(G), p(M1), p(M2), n, p(ctrl), None)
        be.sync()
    finally:
        engine.profile_enable(be.lib, False)
    labels = {nm: c for nm, _, c in engine.profile_fetch(be.lib)}
    assert labels == {'k_adam': 1}, labels
    assert np.array_equal(be.host(G), G0)
    worst = adam_identity(P0, M1_0, M2_0, G0, be.host(P), be.host(M1), be.host(M2), t, hyp, what='k_adam n=%d' % n)
    PC.record_observed('adam_identity', row='adam_step', backend=be.name, n=int(n), route=route, t=int(t),
                       hyper='H0' if tuple(hyp) == H0 else 'H1', **worst)
    return worst
