"""Edge cases of the sort-pool readout (``igmc_amd/csrc/sortpool.hip``) shared by the emulator and the GPU drivers: odd and
large ``k``, subgraph sizes around ``k``, tied sort keys, the largest ``k`` the LDS plan admits -- on subgraphs BUILT TO
ORDER (exact node counts), against ``pyg_ref.DGCNNRSRef`` in FLOAT64 on identical float32 weights, subgraphs and masks.

The bounds that bind are ``parity_checks.DGCNN_OUT_TOL / DGCNN_LOSS_RTOL / DGCNN_GRAD_TOL`` (1.2e-5 / 1.5e-6 / 2.2e-5),
the same as ``run_dgcnn_parity`` asserts inside (the ``worst_grad_err < 1e-3`` lines of the older drivers bind nothing).

What each case reaches in the kernels is said at ``CASES``.  Every case also asserts an INPUT CONDITION: a float32 kernel
and a float64 oracle may order two nearly equal keys differently, so any two keys of a graph (the oracle's float64
``states[3]``) that are not tied (``TIE_EPS``) must differ by more than ``KEY_GAP``.  The seeds in ``CASES`` are the first of
0, 1, 2, ... for which that (and the case's own structural conditions) holds; the tests never search and never skip a graph.
"""
import numpy as np
import scipy.sparse as ssp

import parity_checks as PC
from helpers import batch_to_pyg
from igmc_amd import engine

KEY_GAP = 1e-5
# Two keys this close are a TIE.  Structurally identical nodes -- the twins a case builds, and look-alike nodes that a small
# random graph holds anyway -- have equal keys in exact arithmetic, and the kernels give them equal keys; whether the float64
# oracle gives them the same last bit depends on the host's matrix kernels (a pair that ties exactly on one machine was 7e-18
# apart on another).  1e-12 is thousands of float64 ulps of a key in (-1, 1) and seven orders below KEY_GAP.  Which of two such
# nodes the oracle pools first changes nothing it computes beyond its own rounding: their rows are equal to that precision.
TIE_EPS = 1e-12


# ====================================================================== built-to-order subgraphs
def build_case(sizes, density=0.3, twins=0, seed=0):
    """A rating graph whose link i has a hop-1 enclosing subgraph of EXACTLY ``sizes[i]`` nodes (an int ``n`` stands for
    ``(du, dv) = (n - n // 2, n // 2)``): its own target user and target item, ``du - 1`` private items rated by the target
    user, ``dv - 1`` private users rating the target item -- so ``dv`` users and ``du`` items --, and edges between the
    private users and items drawn with ``density`` (they change no target degree).  Ratings come from 1..5.

    ``twins = t``: the first ``t`` private users of every link rate the target item only, all with one rating: structurally
    identical nodes -- equal states in every layer, exactly tied sort keys in any precision, adjacent in node order."""
    rng = np.random.default_rng(seed)
    rows, cols, vals, links, labels, ns = [], [], [], [], [], []
    nu = nv = 0
    for s in sizes:
        du, dv = (s - s // 2, s // 2) if np.isscalar(s) else s
        assert du >= 1 and dv >= 1 and twins <= dv - 1
        tu, tv = nu, nv
        pu, pv = np.arange(tu + 1, tu + dv), np.arange(tv + 1, tv + du)
        nu, nv = nu + dv, nv + du
        lab = int(rng.integers(0, 5))
        links.append((tu, tv))
        labels.append(lab)
        ns.append(du + dv)
        rows.append([tu]); cols.append([tv]); vals.append([lab + 1])
        rows.append(np.full(len(pv), tu)); cols.append(pv); vals.append(rng.integers(1, 6, len(pv)))
        r = rng.integers(1, 6, len(pu))
        r[:twins] = r[0] if twins else 0
        rows.append(pu); cols.append(np.full(len(pu), tv)); vals.append(r)
        mask = rng.random((len(pu), len(pv))) < density
        mask[:twins] = False
        rr = rng.integers(1, 6, mask.shape)
        iu, iv = np.nonzero(mask)
        rows.append(pu[iu]); cols.append(pv[iv]); vals.append(rr[iu, iv])
    rows, cols = np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)
    A = ssp.csr_matrix((np.concatenate(vals).astype(np.float32), (rows, cols)), shape=(nu, nv))
    return dict(A=A, links=np.array(links, np.int64), link_labels=np.array(labels, np.int64),
                class_values=np.arange(1, 6, dtype=np.float64), h=1, sample_ratio=1.0, mnph=None,
                recs=[None] * len(sizes), sizes=np.array(ns, np.int64), twins=int(twins))


# ====================================================================== the case table
def zero_key_layer(ref):
    """Every sort key becomes ``tanh(bias)``: the pool must be the first k nodes in batch node order."""
    ref.convs[3].basis.zero_()
    ref.convs[3].root.zero_()


KEY_SPREAD = 10.0


def spread_keys(ref):
    """Layer 3's weights times KEY_SPREAD.  With the plain recipe (init + 0.05 randn) the keys of a graph have a standard
    deviation of about 0.05: the graphs of 100+ nodes of a case then hold pairs of distinct keys within KEY_GAP under every
    seed tried (none of 0..59 met the input condition for the three cases that use this; eight to eighteen close pairs a pass at
    seed 0).  Ten times wider pre-activations use the range of tanh and leave a seed within reach; nothing else about the weights
    changes, and the float32 oracle's error beside every recorded value shows what that does to the arithmetic."""
    ref.convs[3].basis.mul_(KEY_SPREAD)
    ref.convs[3].root.mul_(KEY_SPREAD)


# name -> what to build and run.  ``seed`` feeds the builder, the weights and the masks.
CASES = {
    # odd k (Q1 = 31 drops the last pooled row); n = k - 1, k, k + 1; n = 2 (no edge once the target edge is removed); n < 4
    # and n no multiple of 4 (quarter bounds of the rank loop); n either side of a multiple of 64; k_sp_lin_fwd: 54 chunks,
    # 14 a wave -- a second round of ONE chunk, twelve clamped loads
    'around_k_odd': dict(k=63, sizes=[62, 63, 64, 2, 3, 5, 65, 128, 129, 200], drop=(True, False), seed=11, mutate=spread_keys),
    # three fan-in rounds (122 chunks: 13, 13, 5 a wave); B = 17: the second row tile of k_sp_lin_fwd / k_sp_dflat and its
    # arrival counter hold ONE graph
    'k131_B17': dict(k=131, sizes=[131, 130, 132] + [40 + 7 * i for i in range(14)], drop=True, seed=0, mutate=spread_keys),
    # Q2 = 1: two 16-wide chunks, waves 2 and 3 of k_sp_lin_fwd have an empty share
    'k_min_odd': dict(k=11, sizes=[10, 11, 12, 30], drop=True, seed=3),
    # n > 256: a second (thread, quarter) pair in the rank loop; Q1 = 100: a second dzp tile for waves 10..15; about 132 KB
    # of dynamic LDS; slots of the 402-node shape
    'k201_wide': dict(k=201, sizes=[300, 402, 201, 7], density=0.05, drop=True, seed=130, wide=(0, 1), mutate=spread_keys),
    # every key tied: ties go to the lower node index, in the kernel
    'tied_k12': dict(k=12, sizes=[11, 12, 13, 30, 2, 70], drop=False, seed=0, mutate=zero_key_layer, all_tied=True),
    'tied_k63': dict(k=63, sizes=[62, 63, 64, 100], drop=True, seed=0, mutate=zero_key_layer, all_tied=True),
    # groups of five exactly tied keys among distinct ones
    'twins': dict(k=(12, 15, 21), sizes=[(6, 8), (20, 12), (4, 30)], twins=5, drop=False, seed=1),
    # the largest k that create admits for slots of 402 (k is found by the test)
    'k_limit': dict(k=None, sizes=[402, 9], drop=True, seed=16),
}


def runs(name):
    """[(k, drop)] of a case."""
    spec = CASES[name]
    ks = spec['k'] if isinstance(spec['k'], tuple) else (spec['k'],)
    drops = spec['drop'] if isinstance(spec['drop'], tuple) else (spec['drop'],)
    return [(k, dr) for k in ks for dr in drops]


def tie_rule(spec):
    """Which exact ties the case builds (``assert_key_gaps``)."""
    return 'all' if spec.get('all_tied') else spec.get('twins', 0)


def make(name):
    spec = CASES[name]
    return build_case(spec['sizes'], density=spec.get('density', 0.3), twins=spec.get('twins', 0), seed=spec['seed'])


# ====================================================================== oracle
def pool_order(keys):
    """Sort-pool order of one graph's keys: descending, ties (``canon``) by ascending node index."""
    return np.argsort(-canon(keys), kind='stable')


def canon(kg):
    """One graph's keys with every group of keys within TIE_EPS of each other set to one value."""
    order = np.argsort(kg, kind='stable')
    ks = kg[order].copy()
    for j in range(1, len(ks)):
        if ks[j] - ks[j - 1] <= TIE_EPS:
            ks[j] = ks[j - 1]
    out = np.empty_like(kg)
    out[order] = ks
    return out


def assert_key_gaps(keys, node_off, what, tied=0):
    """The input condition: within a graph, two keys are tied (within TIE_EPS) or more than KEY_GAP apart.  ``tied = 'all'``
    (the zeroed key layer): every key of a graph ties; ``tied = t``: nodes 1..t of every graph (the twins) tie."""
    for g in range(len(node_off) - 1):
        kg = keys[node_off[g]:node_off[g + 1]]
        if isinstance(tied, str):
            assert tied == 'all' and np.ptp(kg) <= TIE_EPS, '%s: the keys of graph %d are not all tied' % (what, g)
            continue
        if tied:
            assert np.ptp(kg[1:1 + tied]) <= TIE_EPS, '%s: the twins of graph %d do not tie in the oracle' % (what, g)
        gaps = np.diff(np.sort(kg))
        close = (gaps > TIE_EPS) & (gaps <= KEY_GAP)
        assert not close.any(), ('%s: graph %d has distinct sort keys %.3e apart (input condition: > %.0e); the case needs '
                                 'another seed' % (what, g, gaps[close].min(), KEY_GAP))


def oracle_passes(ref, pyg, lin_mask, edge_mask, ARR):
    """Eval forward and one training forward / backward of ``ref`` on ``pyg``; also the sort keys of both passes."""
    import torch
    from oracle import pyg_ref
    keys = []
    hook = ref.convs[3].register_forward_hook(lambda mod, inp, o: keys.append(torch.tanh(o.detach())[:, 0].numpy().copy()))
    try:
        ref.eval()
        with torch.no_grad():
            eo = ref(pyg)
        ref.train()
        ref.zero_grad()
        to = ref(pyg, edge_mask=edge_mask, lin_mask=torch.from_numpy(lin_mask))
        rl = PC.F_mse(to, pyg.y) + ARR * pyg_ref.arr_loss(ref)
        rl.backward()
    finally:
        hook.remove()
    grads = {key: p.grad.detach().numpy().copy() for key, p in ref.named_parameters()}
    return dict(eval_out=eo.numpy().copy(), train_out=to.detach().numpy().copy(), loss=float(rl.detach()), grads=grads,
                keys_eval=keys[0], keys_train=keys[1])


def prepare(be, case, k, drop, seed, mutate=None, tied=0, R=5, ARR=0.001):
    """Extraction, workspaces, float32 weights, masks and the float64 oracle of one run -- everything but the kernels.  The
    size check comes before anything else; the input condition is asserted on the keys of both oracle passes."""
    import copy
    import torch
    from oracle import pyg_ref
    g, b, d = PC.extract_case(be, case, replay=False)
    assert np.array_equal(np.bincount(d['node_graph'][:d['N']], minlength=d['B']), case['sizes']), \
        (np.bincount(d['node_graph'][:d['N']]), case['sizes'])
    L = 2 * case['h'] + 2
    B = d['B']
    ws = engine.ModelWorkspace(be.lib, be.device, R, 4, L, 0, b.node_capacity, b.edge_capacity, b.max_graphs)
    sp = engine.SortPoolWorkspace(ws, k, max(2, b.node_capacity // b.max_graphs))
    torch.manual_seed(seed)
    ref = pyg_ref.DGCNNRSRef(L, (32, 32, 32, 1), k, R, 4, adj_dropout=0.2 if drop else 0.0, fast=True)
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(0.05 * torch.randn_like(p))
        if mutate is not None:
            mutate(ref)
    sd = {key: v.detach().cpu().numpy().astype(np.float32) for key, v in ref.state_dict().items()}
    flat = np.zeros(sp.n_params, np.float32)
    for key, off in sp.offsets.items():
        a = sd[key].reshape(-1)
        flat[off:off + a.size] = a
    assert sum(v.size for v in sd.values()) == sp.n_params
    rng = np.random.default_rng(seed)
    lin_mask = rng.random((B, 128)) < 0.5
    flags = edge_mask = None
    if drop:
        keep = rng.random(d['E']) >= 0.2
        rev = PC.reverse_positions(d)
        flags = keep.astype(np.uint8) | (keep[rev].astype(np.uint8) << 1)
        edge_mask = torch.from_numpy(keep)
    pyg = batch_to_pyg(d, L)
    ref32 = copy.deepcopy(ref)                       # the float32 oracle: the yardstick for a kernel error near a bound
    o32 = oracle_passes(ref32, pyg, lin_mask, edge_mask, ARR)
    ref = ref.double()                               # float64 oracle on the SAME float32 weights (flattened above)
    pyg.x = pyg.x.double()
    o64 = oracle_passes(ref, pyg, lin_mask, edge_mask, ARR)
    node_off = d['node_off'][:B + 1]
    assert_key_gaps(o64['keys_eval'], node_off, 'eval pass', tied)
    assert_key_gaps(o64['keys_train'], node_off, 'training pass', tied)
    return dict(graph=g, batch=b, d=d, ws=ws, sp=sp, k=int(k), B=int(B), flat=flat, lin_mask=lin_mask, flags=flags, drop=drop,
                ARR=ARR, o64=o64, o32=o32, node_off=node_off)


def run_kernels(be, ctx):
    """Evaluation forward, then one training step with the injected masks; the raw results."""
    sp, b, B = ctx['sp'], ctx['batch'], ctx['B']
    P = be.dev(ctx['flat'])
    out = be.dev(np.zeros(B, np.float32))
    sp.forward(be.ptr(P), b, be.ptr(out), training=False)
    eval_out = be.host(out)
    if ctx['flags'] is not None:
        b.set_edge_flags(ctx['flags'])
    lm = be.dev(ctx['lin_mask'].astype(np.uint8).reshape(-1))
    grad = be.dev(np.zeros(sp.n_params, np.float32))
    loss = be.dev(np.zeros(2, np.float32))
    sp.loss_grad(be.ptr(P), b, be.ptr(out), be.ptr(grad), be.ptr(loss), use_edge_flags=ctx['drop'], lin_mask=be.ptr(lm),
                 ARR=ctx['ARR'])
    return dict(eval_out=eval_out, train_out=be.host(out), loss=be.host(loss), grad=be.host(grad))


def errors(ctx, got, want):
    """The comparisons of ``run_dgcnn_parity``: outputs relative to the batch's peak, loss relative, every gradient tensor
    relative to its peak.  ``got``: raw kernel results, or an oracle's results (then gradients come by name)."""
    sp = ctx['sp']
    worst, worst_key = 0.0, ''
    for key, rgn in want['grads'].items():
        if 'grads' in got:
            t = got['grads'][key]
        else:
            off = sp.offsets[key]
            t = got['grad'][off:off + rgn.size].reshape(rgn.shape)
        err = float(np.abs(t.astype(np.float64) - rgn).max() / max(np.abs(rgn).max(), 1e-6))
        if err > worst:
            worst, worst_key = err, key
    loss = float(got['loss'][0]) if 'grad' in got else got['loss']
    return dict(eval_out_rel=PC.rel_err(got['eval_out'], want['eval_out']),
                train_out_rel=PC.rel_err(got['train_out'], want['train_out']),
                loss_rel=abs(loss - want['loss']) / max(abs(want['loss']), 1e-12),
                worst_grad_rel=worst, worst_grad_tensor=worst_key)


def run_case(be, name, case, k, drop, repeat=False):
    """One row of ``CASES`` through the kernels.  Returns the context (with ``err``: the observed errors)."""
    spec = CASES[name]
    ctx = prepare(be, case, k, drop, spec['seed'], mutate=spec.get('mutate'), tied=tie_rule(spec))
    input_conditions(spec, ctx, case)
    o64, d = ctx['o64'], ctx['d']
    # ---- kernels against the float64 oracle
    got = run_kernels(be, ctx)
    for key in ('eval_out', 'train_out', 'loss', 'grad'):
        assert np.isfinite(got[key]).all(), 'non-finite %s' % key
    if repeat:
        again = run_kernels(be, ctx)
        for key in ('eval_out', 'train_out', 'loss', 'grad'):
            assert got[key].tobytes() == again[key].tobytes(), '%s differs between two runs' % key
    err = errors(ctx, got, o64)
    e32 = errors(ctx, ctx['o32'], o64)
    PC.record_observed('dgcnn_edges', case=name, backend=be.name, k=int(k), B=ctx['B'], N=int(d['N']), dropout=bool(drop),
                       **dict(list(err.items()) + [('f32_oracle_' + key, v) for key, v in e32.items() if key != 'worst_grad_tensor']))
    print('dgcnn_edges %s k=%d drop=%d: %s | float32 oracle: %s' % (name, k, drop, err, e32))
    assert err['eval_out_rel'] < PC.DGCNN_OUT_TOL, err
    assert err['train_out_rel'] < PC.DGCNN_OUT_TOL, err
    assert err['loss_rel'] < PC.DGCNN_LOSS_RTOL, err
    assert err['worst_grad_rel'] < PC.DGCNN_GRAD_TOL, err
    ctx['err'] = err
    return ctx


def input_conditions(spec, ctx, case):
    """The case's own conditions on its inputs, stated in the oracle (the key gaps are asserted by ``prepare``)."""
    o64, d, off, k = ctx['o64'], ctx['d'], ctx['node_off'], ctx['k']
    for g in spec.get('wide', ()):
        # a pool of users only, or of low node indices only, would not notice a rank loop that skips its second stride
        n, nu = int(off[g + 1] - off[g]), int(d['n_users'][g])
        for keys in (o64['keys_eval'], o64['keys_train']):
            pooled = pool_order(keys[off[g]:off[g + 1]])[:k]
            assert (pooled < nu).any() and (pooled >= nu).any(), 'graph %d: the pool holds one side only' % g
            assert (pooled >= 3 * ((n + 3) >> 2)).any(), 'graph %d: no pooled node from the last quarter of the indices' % g
    if case['twins']:
        ctx['twin_flags'] = twin_flags(ctx, case['twins'])


def twin_flags(ctx, t):
    """Where the groups of tied twins (nodes 1..t of every graph) land in the oracle's pool order: (cut by the k boundary --
    some of a group pooled, some not; two of a group in ONE max-pool pair, positions 2q and 2q + 1 below 2 Q1)."""
    off, k = ctx['node_off'], ctx['k']
    cut = paired = False
    for keys in (ctx['o64']['keys_eval'], ctx['o64']['keys_train']):
        for g in range(ctx['B']):
            kg = keys[off[g]:off[g + 1]]
            order = pool_order(kg)
            pos = np.sort(np.nonzero((order >= 1) & (order <= t))[0])
            assert np.array_equal(order[pos], np.arange(1, t + 1)), 'tied twins out of node order in the oracle'
            assert np.array_equal(np.diff(pos), np.ones(t - 1, np.int64)), 'another node ties with the twins of graph %d' % g
            cut |= bool(pos[0] < k <= pos[-1])
            paired |= bool(any(p % 2 == 0 and p + 1 < 2 * (k // 2) for p in pos[:-1]))
    return cut, paired


# ====================================================================== the k limit
def probe_k_limit(ws, nmax, k0=201):
    """Create sort-pool workspaces for k0, k0 + 1, ... until create refuses (creating launches nothing).  Returns the largest
    accepted k; asserts the refusal's message, that nothing below it was refused, and that it stays refused above."""
    import pytest
    k = k0
    while True:
        try:
            sp = engine.SortPoolWorkspace(ws, k, nmax)
        except RuntimeError as e:
            assert 'too large for the LDS plan' in str(e), str(e)
            break
        assert sp.k == k
        del sp
        k += 1
        assert k < 4096, 'create never refuses'
    assert k > k0, 'k = %d is refused already' % k0
    for more in (1, 50):
        with pytest.raises(RuntimeError, match='too large for the LDS plan'):
            engine.SortPoolWorkspace(ws, k + more, nmax)
    return k - 1


def run_k_limit(be):
    """The largest k that ``igmc_sortpool_create`` admits for slots of 402 nodes -- the launches with the most dynamic LDS the
    kernels may ask for -- through the parity runner, once."""
    case = make('k_limit')
    g, b, d = PC.extract_case(be, case, replay=False)
    ws = engine.ModelWorkspace(be.lib, be.device, 5, 4, 2 * case['h'] + 2, 0, b.node_capacity, b.edge_capacity, b.max_graphs)
    k = probe_k_limit(ws, 402)
    del ws, b, g
    (_, drop), = runs('k_limit')
    # (the arena's slots are two nodes wider than its largest subgraph -- the side capacities count the target's own edge --; a
    #  workspace that create refuses at that width fails the run)
    return run_case(be, 'k_limit', case, k, drop)
