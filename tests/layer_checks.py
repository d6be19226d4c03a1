"""Every conv layer of a training launch against float64 on the device's OWN inputs, shared by tests/test_emu_layers.py (host
emulation of the HIP sources) and tests/test_gpu_layers.py (the gfx950 library).

A whole-step tolerance cannot be derived across weight scales -- the error grows through four layers, a head and a backward
pass --, a per-layer one can: after one training launch the stored rows ``h_0 .. h_2`` (``igmc_debug_layer_rows``) and ``h_3`` of
the two centres (``feat``: ``igmc_debug_head_array``) are compared, layer by layer, with

    pre[i,f] = sum_e sum_c h_{l-1}[src_e,c] sum_b att[r_e,b] basis_b[c,f] + sum_c h_{l-1}[i,c] root[c,f] + bias[f]

in float64 over the kept in-edges of the downloaded CSR, ``h_{l-1}`` being the rows the launch itself stored (layer 0: the one-hot
labels).  ``S[i,f]`` is the same sum over the absolute values of its terms.

(a) backstop, derived: ``|h_l - tanh(pre)| <= T + N[i] 2^-24 S[i,f]``.  ``T = 8 * 2^-24`` for the kernels that call ``g2_tanh``
    (prims_checks.check_tanh derives it); the per-layer kernels call ``tanhf`` and get one float32 rounding of a value below 1,
    ``T = 2^-25`` -- no allowance for a library tanh that is not correctly rounded: what it adds must fit beside the sums' error.
    ``N[i] = 3 deg_kept(i) + 6 * 32 (R + 1) + 8`` counts the addends of the longest chain: three bf16 terms per gathered value, six
    term products per element of the transform, the four-term weight composition and the splits.  With the keep bit of the other
    direction in the reference the same comparison must fail (edge flags).
(b) tightness, measured against the reference and never against the kernel: ``q = max over elements of max(err - T, 0) /
    (2^-24 S)``, and ``q_32`` alike (``T = 2^-25``: one rounding) for a plain numpy float32 evaluation of the same layer -- float32
    gather, float32 weight composition and matmuls, float64 tanh rounded once.  ``q_dev <= 4 max(q_32, 1)``: the three-term
    accumulation triples the roundings per accumulated value and the matrix core's block order differs from numpy's.
    What (b) sees, tried on mutated builds (both backends): a gather without its lo plane (q 4.3 in one row) and a tanh of 19
    bits (q 15 .. 28); NOT a truncating bf16 conversion -- three truncations still hold all 24 bits and the dropped term products
    grow from 2^-25 to 2^-23 of a product, inside the margin of 4 --, which prims_checks.check_split catches bit for bit.
(c) tightness without T, for the kernels that call ``g2_tanh``: the kernel's row is ``g2_tanh`` of ITS float32 pre-activation, so that
    pre-activation is among the float32 neighbours of the reference's: ``igmc_debug_g2_prims`` evaluates ``g2_tanh`` -- the form
    of the backend under test -- on the neighbours x_k within 8 * 2^-24 S, and ``p = min {|x_k - pre| : g2_tanh(x_k) == h_l} /
    (2^-24 S)`` is a LOWER bound of the pre-activation's error in which the tanh's own error does not appear (no match: p = inf).
    Over up to 2048 elements a layer with ``|tanh| <= 0.9`` and ``|pre| >= S / 16`` (a flat tanh or a cancelled sum would need
    thousands of neighbours): ``p_dev <= 4 max(p_32, 1)``, ``p_32`` the float32 evaluation's ``|pre_32 - pre| / (2^-24 S)`` over the same
    elements.  Tried on a mutated build: a gather without its lo plane gives p = 4.0 .. 7.7 in every row of the cluster of four at
    scale 1, where q passes 4 in one row only.  (A truncating conversion stays below 4 here as well: see (b).)

Conv parameters (basis, att, root, bias of all four layers) times s in {1, 1/64, 8}: 1/64 puts every pre-activation where the
tanh's quantisation dominates; 8 saturates (``|h| <= 1``, rows of exact +-1 allowed).  At every scale outputs, loss and gradients
are finite and ``igmc_model_check`` is clean, and the whole step is compared with ``oracle/pyg_ref`` in float64 -- asserted at the
suite's tolerances at s = 1, recorded at the other scales.

The batch: seven crafted subgraphs (1,1), (1,40), (15,17), (16,16), (33,64), (65,31), (101,101) on slots of 127 (129 for the
fused dense-layer kernels); a cluster of one workgroup holds 32 rows a side, so its row takes the shapes that fit and two of its
own on both sides of the 16-row bundle.  R = 5 and R = 3, with and without edge flags (``layer3_checks.centre_flags``)."""
import ctypes

import numpy as np

import history_checks as HC
import layer3_checks as L3
import parity_checks as PC

U = 2.0 ** -24
T_G2, T_TANHF, T_F32 = 8 * U, 0.5 * U, 0.5 * U
SCALES = (1.0, 1.0 / 64, 8.0)
SHAPES = [(1, 1), (1, 40), (15, 17), (16, 16), (33, 64), (65, 31), (101, 101)]
SMALL = [s for s in SHAPES if max(s) <= 32] + [(32, 17), (17, 32)]

# family -> (mnph, shapes, expected geometry, hooks, rows by slot (igmc_debug_layer_rows form 0), T)
FAMILIES = {
    'subgraph_wg4': (127, SHAPES, dict(family='subgraph', wg_per_graph=4), {'IGMC_GS_CLUSTER': '4'}, True, T_G2),
    'subgraph_wg1': (31, SMALL, dict(family='subgraph', wg_per_graph=1), {'IGMC_GS_CLUSTER': '1'}, True, T_G2),
    'dense_fused': (128, SHAPES, dict(family='dense_fused', dl_bwd=1, groups=1), {}, False, T_G2),
    'per_layer': (127, SHAPES, dict(family='rows'), {'IGMC_GRAPH_STEP': '0', 'IGMC_DL': '0'}, False, T_TANHF),
}


def case(family, R):
    mnph, shapes, expect, env = FAMILIES[family][:4]
    cap = mnph + 1
    return HC.Case('layers_%s_r%d' % (family, R), mnph, R, len(shapes), (cap, cap), shapes, expect), env


def scaled_params(cr, ws, s):
    """The case's flat parameters with basis, att, root and bias of every conv layer times s (a power of two: exact)."""
    flat = cr.flat.copy()
    for key, off, shape in ws.layout():
        if key.startswith('convs.'):
            flat[off:off + int(np.prod(shape))] *= np.float32(s)
    return flat


def conv_params(ws, flat, l):
    p = {k.split('.')[2]: flat[off:off + int(np.prod(sh))].reshape(sh) for k, off, sh in ws.layout() if k.startswith('convs.%d.' % l)}
    return p['basis'], p['att'], p['root'], p['bias']


def stored_rows(be, ws, b, d, by_slot):
    """-> [h_0, h_1, h_2] as [N, 32] by collated node index"""
    be.sync()
    B, N = d['B'], d['N']
    rows = []
    for l in range(3):
        if by_slot:
            buf = np.full(B * 2 * 128 * 32, np.nan, np.float32)
            be.lib.call('igmc_debug_layer_rows', ws.handle, b.handle, ctypes.c_int(l), ctypes.c_int(0), ctypes.c_void_p(buf.ctypes.data),
                        ctypes.c_int64(buf.size))
            buf = buf.reshape(B, 2, 128, 32)
            h = np.zeros((N, 32), np.float32)
            for g in range(B):
                n0, n1, nu = int(d['node_off'][g]), int(d['node_off'][g + 1]), int(d['n_users'][g])
                h[n0:n0 + nu] = buf[g, 0, :nu]
                h[n0 + nu:n1] = buf[g, 1, :n1 - n0 - nu]
        else:
            h = np.full(N * 32, np.nan, np.float32)
            be.lib.call('igmc_debug_layer_rows', ws.handle, b.handle, ctypes.c_int(l), ctypes.c_int(1), ctypes.c_void_p(h.ctypes.data),
                        ctypes.c_int64(h.size))
            h = h.reshape(N, 32)
        rows.append(h)
    return rows


def feat_rows(be, ws, B):
    buf = np.full(B * 256, np.nan, np.float32)
    be.lib.call('igmc_debug_head_array', ws.handle, 2, ctypes.c_void_p(buf.ctypes.data), B * 256)
    return buf.reshape(B, 2, 4, 32)              # [graph, side, layer, feature]


def edges(d, flags, keep_bit=0):
    N = d['N']
    dst = np.repeat(np.arange(N, dtype=np.int64), np.diff(d['row_ptr']).astype(np.int64))
    src, rel = d['col'].astype(np.int64), d['erel'].astype(np.int64)
    if flags is not None:
        kept = ((flags >> keep_bit) & 1).astype(bool)
        dst, src, rel = dst[kept], src[kept], rel[kept]
    return src, dst, rel


def layer_reference(x, params, src, dst, rel, R):
    """-> (pre, S) in float64 and the float32 evaluation's pre-activation, all [N, 32]; x: the layer's input rows (float32)"""
    basis, att, root, bias = params
    N = x.shape[0]
    x64 = x.astype(np.float64)
    b64, a64 = basis.astype(np.float64), att.astype(np.float64)
    W = np.einsum('rb,bcf->rcf', a64, b64)
    Wabs = np.einsum('rb,bcf->rcf', np.abs(a64), np.abs(b64))
    pre = x64 @ root.astype(np.float64) + bias.astype(np.float64)
    S = np.abs(x64) @ np.abs(root.astype(np.float64)) + np.abs(bias.astype(np.float64))
    W32 = np.einsum('rb,bcf->rcf', att, basis).astype(np.float32)
    pre32 = (x @ root + bias).astype(np.float32)
    for r in range(R):
        sel = rel == r
        T, T32 = np.zeros((N, x.shape[1])), np.zeros((N, x.shape[1]), np.float32)
        np.add.at(T, dst[sel], x64[src[sel]])
        np.add.at(T32, dst[sel], x[src[sel]])
        Ta = np.zeros_like(T)
        np.add.at(Ta, dst[sel], np.abs(x64[src[sel]]))
        pre += T @ W[r]
        S += Ta @ Wabs[r]
        pre32 = (pre32 + T32 @ W32[r]).astype(np.float32)
    return pre, S, pre32


def compare(got, pre, S, n_chain, T):
    """-> (elements beyond the backstop, q, largest err / backstop)"""
    ref = np.tanh(pre)
    err = np.abs(got.astype(np.float64) - ref)
    bound = T + n_chain[:, None] * U * S
    q = float((np.maximum(err - T, 0.0) / (U * S)).max())
    return err > bound, q, float((err / bound).max())


def run(cr, family, drop, s):
    """One training launch of the case's target batch at conv scale s -> what ``check_layers`` and ``check_whole_step`` look at."""
    with L3.flags_injected():
        b, ws = cr.pair()
        flat = scaled_params(cr, ws, s)
        res = HC.run_step(cr, b, ws, cr.target, drop, P=cr.be.dev(flat))
        HC.assert_finite(res, '%s s=%g' % (cr.case.id, s))
        cr.be.lib.call('igmc_model_check', ws.handle, None)
        res.update(b=b, flat=flat, flags=HC.edge_flags_by_id(res['d']) if drop else None)
        res['rows'] = stored_rows(cr.be, ws, b, res['d'], FAMILIES[family][4])
        res['feat'] = feat_rows(cr.be, ws, cr.case.B)
    return res


def inverted_error(be, got, pre, S, seed):
    """(c) of the module docstring -> (p per chosen element, the chosen elements' flat indices)"""
    import prims_checks as PR
    t = np.tanh(pre)
    ok = np.flatnonzero((np.abs(t) <= 0.9) & (np.abs(pre) >= S / 16) & (np.abs(pre) >= 2.0 ** -100))
    pick = np.random.default_rng(seed).permutation(ok)[:2048]
    x0 = pre.reshape(-1)[pick].astype(np.float32)
    # neighbours of float32(pre) out to 8 * 2^-24 S: a unit in the last place of x exceeds 2^-24 |x| >= 2^-24 S / 16, so 8 * 16 of them
    K = 130
    k = np.arange(-K, K + 1, dtype=np.int64)
    mag = PR.bits(np.abs(x0)).astype(np.int64)[:, None] + k[None, :]           # (same sign: K places are far less than |pre|)
    assert (mag > 0).all()
    xk = np.copysign(PR.f32(mag.astype(np.uint32).reshape(-1)), np.repeat(x0, k.size)).astype(np.float32)
    hk = PR.probe_f32(be, PR.TANH, xk).reshape(len(pick), k.size)
    dist = np.abs(xk.reshape(len(pick), k.size).astype(np.float64) - pre.reshape(-1)[pick][:, None])
    dist[hk != got.reshape(-1)[pick][:, None]] = np.inf
    return dist.min(1) / (U * S.reshape(-1)[pick]), pick


def check_layers(cr, res, family, drop, s):
    """(a), (b) and (c) of the module docstring for every layer of one launch; -> [(layer, q_dev, q_32, worst err / backstop)]"""
    d, ws, R, B, T = res['d'], res['ws'], cr.case.R, cr.case.B, FAMILIES[family][5]
    N = d['N']
    rows, feat = res['rows'], res['feat']
    src, dst, rel = edges(d, res['flags'])
    deg = np.bincount(dst, minlength=N)
    n_chain = 3 * deg + 6 * 32 * (R + 1) + 8
    isolated = deg == 0
    assert isolated.any() and (~isolated).any()
    centres = np.concatenate([d['node_off'][:-1], d['node_off'][:-1] + d['n_users']]).astype(np.int64)       # [side][graph]
    assert (d['node_label'][centres[:B]] == 0).all() and (d['node_label'][centres[B:]] == 1).all()
    x0 = np.zeros((N, cr.L), np.float32)
    x0[np.arange(N), d['node_label']] = 1.0
    inputs = [x0] + rows
    for l in range(3):
        assert np.isfinite(rows[l]).all(), 'h_%d: non-finite stored rows' % l
        assert (np.abs(rows[l]) <= 1.0).all(), 'h_%d: |h| exceeds 1' % l
        # the readout's copy of the centre rows is the stored row
        assert np.array_equal(feat[:, 0, l], rows[l][centres[:B]]) and np.array_equal(feat[:, 1, l], rows[l][centres[B:]]), \
            'feat does not hold the stored h_%d of the centre rows' % l
    assert np.isfinite(feat).all() and (np.abs(feat) <= 1.0).all()
    out = []
    for l in range(4):
        pre, S, pre32 = layer_reference(inputs[l], conv_params(ws, res['flat'], l), src, dst, rel, R)
        if l < 3:
            got, sel = rows[l], np.arange(N)
        else:
            got, sel = np.concatenate([feat[:, 0, 3], feat[:, 1, 3]]), centres
        what = '%s drop=%s s=%g layer %d' % (cr.case.id, drop, s, l)
        bad, q_dev, worst = compare(got, pre[sel], S[sel], n_chain[sel], T)
        h32 = np.tanh(pre32[sel].astype(np.float64)).astype(np.float32)
        _, q_32, _ = compare(h32, pre[sel], S[sel], n_chain[sel], T_F32)
        iso = isolated[sel]
        worst_iso = float((np.abs(got[iso].astype(np.float64) - np.tanh(pre[sel][iso])) / (T + n_chain[sel][iso][:, None] * U * S[sel][iso])).max())
        print('%s: q_dev %.3f q_32 %.3f worst err / backstop %.4f (rows without a kept in-edge: %.4f)' % (what, q_dev, q_32, worst, worst_iso))
        PC.record_observed('layer_accuracy', case=cr.case.id, family=family, backend=cr.be.name, dropout=bool(drop), scale=float(s), layer=l,
                           q_dev=q_dev, q_32=q_32, worst_err_over_backstop=worst, saturated_rows=int((np.abs(got) == 1).all(1).sum()))
        out.append((l, q_dev, q_32, worst))
        assert not bad.any(), '%s: %d of %d elements beyond T + N 2^-24 S (first at [row, f] = %s; worst err / bound %.3f)' % (
            what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), worst)
        assert worst_iso <= 1.0
        assert q_dev <= 4 * max(q_32, 1.0), '%s: q_dev %.3f beyond 4 max(q_32 = %.3f, 1): the layer is not at float32 accuracy' % (what, q_dev, q_32)
        if T == T_G2:
            p, pick = inverted_error(cr.be, got, pre[sel], S[sel], 7 + l)
            p_dev = float(p.max()) if p.size else 0.0
            p_32 = float((np.abs(pre32[sel].astype(np.float64) - pre[sel]) / (U * S[sel])).reshape(-1)[pick].max()) if p.size else 0.0
            print('%s: p_dev %.3f p_32 %.3f over %d elements' % (what, p_dev, p_32, p.size))
            PC.record_observed('layer_accuracy_inverted', case=cr.case.id, family=family, backend=cr.be.name, dropout=bool(drop), scale=float(s),
                               layer=l, p_dev=p_dev, p_32=p_32, elements=int(p.size))
            assert s != 1.0 or p.size >= (256 if l < 3 else 64), '%s: too few elements for the inversion (%d)' % (what, p.size)      # (layer 3: the centres)
            assert p_dev <= 4 * max(p_32, 1.0), '%s: p_dev %.3f beyond 4 max(p_32 = %.3f, 1): the pre-activation is not at float32 accuracy' % (
                what, p_dev, p_32)
        if drop and l in (1, 2) and s == 1.0:            # the check does see a wrong keep bit
            L3.assert_one_way_centre_edges(d)
            s1, d1, r1 = edges(d, res['flags'], keep_bit=1)
            pre1, S1, _ = layer_reference(inputs[l], conv_params(ws, res['flat'], l), s1, d1, r1, R)
            bad1, _, _ = compare(got, pre1[sel], S1[sel], 3 * np.bincount(d1, minlength=N)[sel] + 6 * 32 * (R + 1) + 8, T)
            assert bad1.any(), '%s: the rows also match the keep bit of the other direction: the check cannot see it' % what
    return out


def check_whole_step(cr, res, family, drop, s):
    """The launch against ``oracle/pyg_ref`` in float64 with the conv parameters scaled alike: asserted at the suite's tolerances at
    s = 1, recorded at the other scales."""
    import torch
    from helpers import batch_to_pyg
    from oracle import pyg_ref
    d, B = res['d'], cr.case.B
    m = PC.make_ref_model(cr.L, cr.case.R, seed=3, adj_dropout=0.2 if drop else 0.0).to(torch.float64)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.startswith('convs.'):
                p.mul_(s)
    assert np.array_equal(PC.flatten_params(res['ws'], m), res['flat']), 'the oracle does not hold the launch\'s parameters'
    pyg = batch_to_pyg(d, cr.L)
    pyg.x, pyg.y = pyg.x.to(torch.float64), pyg.y.to(torch.float64)
    _, ev = pyg_ref.eval_sse(m, pyg)
    edge_mask = torch.from_numpy((res['flags'] & 1).astype(bool)) if drop else None
    rl, ro, rg = pyg_ref.loss_and_grads(m, pyg, ARR=HC.ARR, edge_mask=edge_mask, lin_mask=torch.from_numpy(cr.lin[res['order']]))
    grads = PC.unflatten_grads(res['ws'], res['grad'])
    worst, key = 0.0, ''
    for k, r in rg.items():
        r = r.numpy().astype(np.float64)
        e = float(np.abs(grads[k] - r).max() / max(np.abs(r).max(), 1e-6))
        if e > worst:
            worst, key = e, k
    e_ev, e_out = PC.rel_err(res['ev'][:B], ev.numpy().astype(np.float64)), PC.rel_err(res['out'][:B], ro.numpy().astype(np.float64))
    e_loss = abs(float(res['loss'][0]) - float(rl)) / max(abs(float(rl)), 1e-12)
    print('%s drop=%s s=%g whole step: eval out %.3e train out %.3e loss %.3e worst grad %.3e (%s)' % (cr.case.id, drop, s, e_ev, e_out, e_loss, worst, key))
    PC.record_observed('layer_whole_step', case=cr.case.id, family=family, backend=cr.be.name, dropout=bool(drop), scale=float(s),
                       eval_out_rel=e_ev, train_out_rel=e_out, loss_rel=e_loss, worst_grad_rel=worst, worst_grad_tensor=key)
    if s == 1.0:
        assert e_ev < PC.OUT_TOL and e_out < PC.OUT_TOL, (e_ev, e_out)
        assert e_loss < PC.LOSS_RTOL, e_loss
        assert worst < PC.GRAD_TOL, (key, worst)
    return e_ev, e_out, e_loss, worst
