"""Pointer-level Python handles over the C ABI (``include/igmc_hip.h``).

Everything here works on raw device addresses (ints), so it is independent of how the buffers
were allocated (torch tensors in the product; the kernel-logic tests drive the host emulation
build of the same sources with numpy buffers).  The reference-shaped API lives one level up in
``igmc_amd.util_functions`` / ``igmc_amd.models`` / ``igmc_amd.train_eval``.
"""
import ctypes as C

import numpy as np

from . import _lib


def _p(x):
    """int / None / numpy array -> c_void_p"""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    return C.c_void_p(int(x))


class Graph(object):
    """Rating graph resident in HBM (replaces SparseRowIndexer/SparseColIndexer,
    reference util_functions.py:20-66)."""

    def __init__(self, A, device=0, lib=None):
        self.lib = lib or _lib.load()
        A = A.tocsr()
        A.sum_duplicates()
        A.sort_indices()
        self.n_users, self.n_items = A.shape
        indptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
        indices = np.ascontiguousarray(A.indices, dtype=np.int32)
        vals = np.asarray(A.data)
        if len(vals) and (vals.min() < 0 or vals.max() > 255 or np.any(vals != np.round(vals))):
            raise ValueError('adjacency values must be rating-label + 1 (small non-negative integers)')
        rating = np.ascontiguousarray(vals, dtype=np.uint8)
        self.nnz = int((rating != 0).sum())
        self.max_rel = int(rating.max()) - 1 if len(rating) else 0
        h = C.c_void_p()
        self.lib.call('igmc_graph_create', self.n_users, self.n_items, len(indices), _p(indptr), _p(indices),
                      _p(rating), device, C.byref(h))
        self.handle = h
        self.device = device

    def hbm_bytes(self):
        return int(self.lib.igmc_graph_hbm_bytes(self.handle))

    @classmethod
    def _from_handle(cls, handle, device, lib):
        self = cls.__new__(cls)
        self.lib, self.handle, self.device = lib, handle, device
        i = self.info()
        self.n_users, self.n_items, self.nnz, self.max_rel = i['n_users'], i['n_items'], i['nnz'], i['max_rel']
        return self

    def info(self):
        """The six sizes of ``igmc_graph_info``."""
        out = np.zeros(6, np.int64)
        self.lib.call('igmc_graph_info', self.handle, _p(out))
        return dict(zip(('n_users', 'n_items', 'nnz', 'max_rel', 'max_deg_u', 'max_deg_v'), (int(x) for x in out)))

    def download(self):
        """The resident arrays on the host: ``u_ptr``, ``u_idx``, ``u_rel`` (rows by (relation, item)), ``v_ptr``, ``v_idx``,
        ``v_rel`` (columns by (relation, user))."""
        i = self.info()
        d = dict(u_ptr=np.zeros(i['n_users'] + 1, np.int32), u_idx=np.zeros(i['nnz'], np.int32), u_rel=np.zeros(i['nnz'], np.uint8),
                 v_ptr=np.zeros(i['n_items'] + 1, np.int32), v_idx=np.zeros(i['nnz'], np.int32), v_rel=np.zeros(i['nnz'], np.uint8))
        self.lib.call('igmc_graph_download', self.handle, _p(d['u_ptr']), _p(d['u_idx']), _p(d['u_rel']), _p(d['v_ptr']),
                      _p(d['v_idx']), _p(d['v_rel']))
        return d

    def to_scipy(self):
        """The rating matrix as a CSR with values rating label + 1 (what the constructor takes)."""
        import scipy.sparse as ssp
        d = self.download()
        A = ssp.csr_matrix((d['u_rel'].astype(np.float32) + 1.0, d['u_idx'], d['u_ptr']), shape=(self.n_users, self.n_items))
        A.sort_indices()
        return A

    def updated(self, users, items, ratings, n_users=None, n_items=None, stream=None):
        """A NEW graph: this one after ``A[users[j], items[j]] = ratings[j]`` for j = 0, 1, .. in order (``igmc_graph_apply``:
        ratings are rating label + 1, 0 removes the entry, the last assignment of a pair wins), built on the device; this
        graph and everything bound to it stay as they are.  ``users`` / ``items`` / ``ratings``: integer arrays of one length,
        host (numpy, lists) or device (torch).  ``n_users`` / ``n_items``: the new sizes, by default the larger of the present
        size and the greatest id + 1 -- ids beyond the graph create new, otherwise empty, rows and columns."""
        keep = []
        u, mu = self._change_array(users, np.int32, 'users', keep)
        v, mv = self._change_array(items, np.int32, 'items', keep)
        r, _ = self._change_array(ratings, np.uint8, 'ratings', keep)
        if not len(u) == len(v) == len(r):
            raise ValueError('users, items and ratings differ in length')
        n_users = max(self.n_users, mu + 1) if n_users is None else int(n_users)
        n_items = max(self.n_items, mv + 1) if n_items is None else int(n_items)
        if stream is None and keep and hasattr(keep[0], 'data_ptr'):
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        h = C.c_void_p()
        ptr = lambda a: _p(a.data_ptr() if hasattr(a, 'data_ptr') else a) if len(a) else None
        self.lib.call('igmc_graph_apply', self.handle, n_users, n_items, ptr(u), ptr(v), ptr(r), len(u), _p(stream), C.byref(h))
        return Graph._from_handle(h, self.device, self.lib)

    def _change_array(self, x, dtype, what, keep):
        """``x`` as a contiguous array of ``dtype`` where the library reads it (the GPU for the product library; the host
        emulation build of the tests reads numpy memory) and its greatest entry (-1: none)."""
        if hasattr(x, 'data_ptr'):          # a torch tensor, host or device
            import torch
            if x.dim() != 1 or x.dtype.is_floating_point or x.dtype == torch.bool:
                raise ValueError('%s: a 1-D integer array' % what)
            top = int(x.max().item()) if x.numel() else -1
            low = int(x.min().item()) if x.numel() else 0
            if dtype == np.uint8 and (low < 0 or top > 255):
                raise ValueError('ratings must be rating label + 1 in 1..255, or 0 to remove')
            t = x.to(device='cuda:%d' % self.device, dtype=torch.uint8 if dtype == np.uint8 else torch.int32).contiguous()
            keep.append(t)
            return t, top
        a = np.asarray(x)
        if a.ndim != 1 or (a.size and a.dtype.kind not in 'iu'):
            raise ValueError('%s: a 1-D integer array' % what)
        top = int(a.max()) if a.size else -1
        if dtype == np.uint8 and a.size and (int(a.min()) < 0 or top > 255):
            raise ValueError('ratings must be rating label + 1 in 1..255, or 0 to remove')
        if a.size and (int(a.min()) < -2 ** 31 or top >= 2 ** 31):
            raise ValueError('%s: ids must fit int32' % what)
        a = np.ascontiguousarray(a, dtype=dtype)
        if self.lib is _lib._cached:        # the product library reads device memory
            import torch
            t = torch.from_numpy(a).to('cuda:%d' % self.device)
            keep.append(t)
            return t, top
        keep.append(a)
        return a, top

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.igmc_graph_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch(object):
    """Arena for one extracted + collated batch of enclosing subgraphs."""

    def __init__(self, graph, max_graphs, hop=1, max_nodes_per_hop=None):
        self.lib = graph.lib
        self.graph = graph
        self.max_graphs = int(max_graphs)
        self.hop = int(hop)
        self.mnph = -1 if max_nodes_per_hop is None else int(max_nodes_per_hop)
        h = C.c_void_p()
        self.lib.call('igmc_batch_create', graph.handle, self.max_graphs, self.hop, self.mnph, C.byref(h))
        self.handle = h
        info = self.info()
        self.node_capacity, self.edge_capacity = info.node_capacity, info.edge_capacity
        self.num_labels = info.num_labels
        self.B = 0

    def extract(self, link_u, link_v, link_y, link_idx, first, B, sample_ratio=1.0, seed=0, epoch=0, stream=None):
        self.lib.call('igmc_extract_batch', self.graph.handle, self.handle, _p(link_u), _p(link_v), _p(link_y),
                      _p(link_idx), int(first), int(B), float(sample_ratio), int(seed) & (2 ** 64 - 1),
                      int(epoch) & (2 ** 64 - 1), _p(stream))
        self.B = int(B)

    def extract_cached(self, cache, link_y, link_idx, first, B, stream=None):
        """Batch ``link_idx[first:first+B]`` from a device-resident node-set cache (``igmc_extract_batch_cached``);
        ``cache`` = dict of device addresses uoff, unodes, udist, voff, vnodes, vdist."""
        self.lib.call('igmc_extract_batch_cached', self.graph.handle, self.handle, _p(cache['uoff']), _p(cache['unodes']),
                      _p(cache['udist']), _p(cache['voff']), _p(cache['vnodes']), _p(cache['vdist']), _p(link_y),
                      _p(link_idx), int(first), int(B), _p(stream))
        self.B = int(B)

    def extract_replay(self, u_lists, v_lists, u_dists, v_dists, ys, stream=None):
        """Parity mode: node sets given per graph (target first)."""
        B = len(u_lists)
        uoff = np.zeros(B + 1, np.int32)
        voff = np.zeros(B + 1, np.int32)
        uoff[1:] = np.cumsum([len(x) for x in u_lists])
        voff[1:] = np.cumsum([len(x) for x in v_lists])
        un = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32) for x in u_lists]))
        vn = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32) for x in v_lists]))
        ud = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint8) for x in u_dists]))
        vd = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint8) for x in v_dists]))
        y = np.ascontiguousarray(np.asarray(ys, np.float32))
        self.lib.call('igmc_extract_batch_replay', self.graph.handle, self.handle, B, _p(un), _p(ud), _p(uoff),
                      _p(vn), _p(vd), _p(voff), _p(y), _p(stream))
        self.B = B

    def edge_dropout(self, p, force_undirected=False, seed=0, step=0, stream=None):
        self.lib.call('igmc_batch_edge_dropout', self.handle, float(p), int(bool(force_undirected)),
                      int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), _p(stream))

    def set_edge_flags(self, flags):
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        self.lib.call('igmc_batch_set_edge_flags', self.handle, _p(flags), len(flags))

    def clear_edge_flags(self):
        self.lib.call('igmc_batch_clear_edge_flags', self.handle)

    def set_side_features(self, ptr, n_side):
        self.lib.call('igmc_batch_set_side_features', self.handle, _p(ptr), int(n_side))

    def bind_side_source(self, ptr, n_side):
        """Dataset-wide [n_links, n_side] side-feature matrix: every later ``extract`` gathers the batch's rows on the
        device (``igmc_batch_bind_side_source``)."""
        self.lib.call('igmc_batch_bind_side_source', self.handle, _p(ptr), int(n_side))

    def bind_side_tables(self, u_ptr, n_u_rows, fu, v_ptr, n_v_rows, fv):
        """Per-node side-feature tables ``[n_u_rows, fu]`` / ``[n_v_rows, fv]``: every later ``extract`` / ``extract_cached``
        gathers the rows of the batch's target nodes on the device, by the ids the extraction left in the arena; ids beyond a
        table read zeros (``igmc_batch_bind_side_tables``).  All zero / None unbinds."""
        self.lib.call('igmc_batch_bind_side_tables', self.handle, _p(u_ptr), int(n_u_rows), int(fu), _p(v_ptr), int(n_v_rows),
                      int(fv))

    def dense_layers(self, ws):
        """True when the dense per-layer kernels take the conv layers of this arena with workspace ``ws``."""
        return bool(self.lib.cdll.igmc_model_dense_layers(ws.handle, self.handle, int(self.B or self.max_graphs)))

    def want_transposed(self):
        """Keep the transposed dense blocks too (dense-layer kernels for models the subgraph kernel does not take)."""
        self.lib.call('igmc_batch_want_transposed', self.handle)

    def set_lean(self, lean=True):
        """Lean extraction: stop after the dense induced blocks (what the matrix-core subgraph kernel reads); the
        collated CSR is emitted on demand (``igmc_batch_set_lean``)."""
        self.lib.call('igmc_batch_set_lean', self.handle, int(bool(lean)))

    def assume_size(self, B):
        """The arena holds ``B`` subgraphs extracted by a replayed launch (``igmc_batch_assume_size``)."""
        self.lib.call('igmc_batch_assume_size', self.handle, int(B))
        self.B = int(B)

    def info(self, stream=None):
        info = _lib.BatchInfo()
        self.lib.call('igmc_batch_get_info', self.handle, C.byref(info), _p(stream))
        return info

    def device_ptr(self, name):
        return self.lib.igmc_batch_device_ptr(self.handle, _lib.BUF[name])

    def download(self, stream=None):
        """Host copy of the collated batch (synchronises)."""
        info = self.info(stream)
        if info.overflow:
            raise RuntimeError('batch arena overflow: N=%d E=%d exceed the capacity (%d, %d)' % (
                info.num_nodes, info.num_edges, info.node_capacity, info.edge_capacity))
        B, N, E = info.num_graphs, info.num_nodes, info.num_edges
        out = dict(
            node_off=np.zeros(B + 1, np.int32), n_users=np.zeros(B, np.int32),
            node_label=np.zeros(N, np.uint8), node_gid=np.zeros(N, np.int32), node_graph=np.zeros(N, np.int32),
            row_ptr=np.zeros(N + 1, np.int32), col=np.zeros(E, np.int32), erel=np.zeros(E, np.uint8),
            elab=np.zeros(E, np.uint8), eflag=np.zeros(E, np.uint8), y=np.zeros(B, np.float32))
        self.lib.call('igmc_batch_download', self.handle, _p(out['node_off']), _p(out['n_users']),
                      _p(out['node_label']), _p(out['node_gid']), _p(out['node_graph']), _p(out['row_ptr']),
                      _p(out['col']), _p(out['erel']), _p(out['elab']), _p(out['eflag']), _p(out['y']), _p(stream))
        out['B'], out['N'], out['E'] = B, N, E
        return out

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.igmc_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchSet(object):
    """A group of arenas of one geometry that ``igmc_extract_group`` fills in one launch per stage."""

    def __init__(self, arenas):
        self.arenas = list(arenas)
        self.lib = self.arenas[0].lib
        hs = (C.c_void_p * len(self.arenas))(*[a.handle for a in self.arenas])
        h = C.c_void_p()
        self.lib.call('igmc_batch_set_create', C.cast(hs, C.c_void_p), len(self.arenas), C.byref(h))
        self.handle = h

    def extract(self, count, link_u, link_v, link_y, link_idx, sel0, B, sample_ratio=1.0, seed=0, drop_p=0.0,
                force_undirected=False, drop_seed=0, stream=None):
        """Batches sel0 + 2 i (i < count; selectors of the device-side step control) into arenas 0 .. count-1, followed by
        their edge dropout when ``drop_p`` > 0."""
        self.lib.call('igmc_extract_group', self.arenas[0].graph.handle, self.handle, int(count), _p(link_u), _p(link_v),
                      _p(link_y), _p(link_idx), int(sel0), int(B), float(sample_ratio), int(seed) & (2 ** 64 - 1),
                      float(drop_p), int(bool(force_undirected)), int(drop_seed) & (2 ** 64 - 1), _p(stream))
        for a in self.arenas[:count]:
            a.B = int(B)

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.cdll.igmc_batch_set_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ModelWorkspace(object):
    """Model geometry + activation/gradient workspace; knows the flat parameter layout."""

    PARAM_KINDS = ('BASIS', 'ROOT', 'BIAS', 'ATT')

    def __init__(self, lib, device, num_relations, num_bases, num_labels, n_side, max_nodes, max_edges, max_graphs):
        self.lib = lib
        self.R, self.Bs, self.L, self.S = int(num_relations), int(num_bases), int(num_labels), int(n_side)
        self.max_nodes, self.max_edges, self.max_graphs = int(max_nodes), int(max_edges), int(max_graphs)
        h = C.c_void_p()
        lib.call('igmc_model_create', int(device), self.R, self.Bs, self.L, self.S, self.max_nodes,
                 self.max_edges, self.max_graphs, C.byref(h))
        self.handle = h
        self.n_params = int(lib.igmc_param_count(h))

    def layout(self):
        """[(state_dict key, offset, shape)] in flat-buffer order (reference state_dict names)."""
        out = []
        for l in range(4):
            fin = self.L if l == 0 else 32
            shapes = dict(BASIS=(self.Bs, fin, 32), ROOT=(fin, 32), BIAS=(32,), ATT=(self.R, self.Bs))
            for kind, key in (('BASIS', 'basis'), ('ROOT', 'root'), ('BIAS', 'bias'), ('ATT', 'att')):
                cnt = C.c_int64()
                off = self.lib.igmc_param_offset(self.handle, l, _lib.P[kind], C.byref(cnt))
                assert cnt.value == int(np.prod(shapes[kind]))
                out.append(('convs.%d.%s' % (l, key), int(off), shapes[kind]))
        D = 256 + self.S
        for kind, key, shape in (('LIN1_W', 'lin1.weight', (128, D)), ('LIN1_B', 'lin1.bias', (128,)),
                                 ('LIN2_W', 'lin2.weight', (1, 128)), ('LIN2_B', 'lin2.bias', (1,))):
            cnt = C.c_int64()
            off = self.lib.igmc_param_offset(self.handle, 0, _lib.P[kind], C.byref(cnt))
            assert cnt.value == int(np.prod(shape))
            out.append((key, int(off), shape))
        return out

    def forward(self, params, batch, out, training=False, use_edge_flags=False, lin_mask=None, seed=0, step=0,
                multiply_by=1.0, stream=None):
        self.lib.call('igmc_model_forward', self.handle, _p(params), batch.handle, int(bool(training)),
                      int(bool(use_edge_flags)), _p(lin_mask), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1),
                      float(multiply_by), _p(out), _p(stream))

    def backward(self, params, batch, gout, grad, multiply_by=1.0, stream=None):
        self.lib.call('igmc_model_backward', self.handle, _p(params), batch.handle, _p(gout), float(multiply_by),
                      _p(grad), _p(stream))

    def loss_grad(self, params, batch, out, grad, loss, use_edge_flags=False, lin_mask=None, seed=0, step=0,
                  multiply_by=1.0, ARR=0.0, grad_scale=None, arr_scale=1.0, stream=None):
        if grad_scale is None:
            grad_scale = 1.0 / batch.B
        self.lib.call('igmc_model_loss_grad', self.handle, _p(params), batch.handle, int(bool(use_edge_flags)),
                      _p(lin_mask), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), float(multiply_by),
                      float(ARR), float(grad_scale), float(arr_scale), _p(out), _p(grad), _p(loss), _p(stream))

    def pair_loss_grad(self, params, batch, out, gout, grad, stats, use_edge_flags=False, lin_mask=None, seed=0, step=0,
                       multiply_by=1.0, ARR=0.0, mse_weight=1.0, stream=None):
        """One pair step's loss and gradient on a batch of (positive, negative) slots (``igmc_pair_loss_grad``): ``out`` /
        ``gout`` float32 ``[B]``, ``grad`` the flat gradient, ``stats`` float64 ``[5]``."""
        self.lib.call('igmc_pair_loss_grad', self.handle, _p(params), batch.handle, int(bool(use_edge_flags)), _p(lin_mask),
                      int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), float(multiply_by), float(ARR), float(mse_weight),
                      _p(out), _p(gout), _p(grad), _p(stats), _p(stream))

    def dense_path(self, batch, B):
        """True when forward / loss_grad / train_step on (batch arena, B) take the matrix-core subgraph kernel."""
        return bool(self.lib.igmc_model_dense_path(self.handle, batch.handle, int(B)))

    def step_form(self, batch, B):
        """Kernels of a training step on (batch arena, B): 1 subgraph kernel, 2 dense-layer kernels, 3 those in their
        group-split form, 0 per-layer kernels (igmc_model_step_form)."""
        return int(self.lib.igmc_model_step_form(self.handle, batch.handle, int(B)))

    def l3_vectors(self, batch, B):
        """Non-zero when a training step on (batch arena, B) hands layer 3's weight gradient to the tail as centre vectors
        (igmc_debug_l3_vectors): the cluster member that owns the item centre; 0: per-workgroup tables."""
        fn = self.lib.cdll.igmc_debug_l3_vectors
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int]
        return int(fn(self.handle, batch.handle, int(B)))

    GEOMETRY_KEYS = ('form', 'family', 'wg_per_graph', 'grid', 'nqu', 'nqv', 'groups', 'gsplit', 'tables', 'kp', 'dl_bwd')
    FAMILIES = ('rows', 'subgraph', 'dense_fused', 'dense_layer')

    def step_geometry(self, batch, B):
        """Launch geometry of a training step on (batch arena, B) (igmc_model_step_geometry): ``family`` is one of
        FAMILIES; ``wg_per_graph`` / ``grid`` of the subgraph kernel, ``nqu`` / ``nqv`` workgroups of a subgraph's sides
        in the dense layers, ``groups`` relation groups and ``gsplit`` both at once, ``tables`` a backward that leaves
        relation-space tables, ``kp`` the subgraph kernel's padded plane extent, ``dl_bwd`` the one-launch dense backward."""
        n = len(self.GEOMETRY_KEYS)
        out = (C.c_int32 * n)()
        self.lib.call('igmc_model_step_geometry', self.handle, batch.handle, int(B), C.cast(out, C.c_void_p), n)
        g = dict(zip(self.GEOMETRY_KEYS, [int(x) for x in out]))
        g['family'] = self.FAMILIES[g['family']]
        return g

    def adam_step(self, params, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8,
                  weight_decay=0.0, stream=None):
        self.lib.call('igmc_adam_step', _p(params), _p(grad), _p(exp_avg), _p(exp_avg_sq), self.n_params, int(step),
                      float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), _p(stream))

    def sse_accumulate(self, out, batch, acc, stream=None, ctrl=None):
        """``ctrl``: the control block of a grouped evaluation pipeline -- its tick in the same launch."""
        if ctrl is not None:
            self.lib.call('igmc_sse_accumulate_tick', _p(out), batch.handle, _p(acc), _p(ctrl), _p(stream))
        else:
            self.lib.call('igmc_sse_accumulate', _p(out), batch.handle, _p(acc), _p(stream))

    def scores_store(self, out, batch, acc, scores, labels, n, err, first=-1, stream=None, ctrl=None):
        """``sse_accumulate`` that also files the batch's outputs / labels at ``first + g`` of ``scores`` / ``labels``
        (``igmc_scores_store``); ``first`` = -1: the position the batch's extraction left in its arena."""
        self.lib.call('igmc_scores_store', _p(out), batch.handle, _p(acc), _p(scores), _p(labels), int(n), int(first),
                      _p(ctrl), _p(err), _p(stream))

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.igmc_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def adam_step(lib, params, grad, exp_avg, exp_avg_sq, n, step, lr, beta1=0.9, beta2=0.999, eps=1e-8,
              weight_decay=0.0, stream=None):
    """Fused Adam over a flat buffer (no model workspace needed)."""
    lib.call('igmc_adam_step', _p(params), _p(grad), _p(exp_avg), _p(exp_avg_sq), int(n), int(step), float(lr),
             float(beta1), float(beta2), float(eps), float(weight_decay), _p(stream))


def select_extremes(keys, num, grid=0, lib=None, stream=None):
    """The ``num`` first and the ``num`` last (reversed) of the stable ascending order of a device float32 vector
    (``igmc_select_extremes``; reference ``train_eval.py:262-272``).  Returns device tensors ``(idx_low, idx_high, key_low,
    key_high)`` of ``min(len(keys), num)`` entries; the keys never leave the device."""
    import torch
    lib = lib or _lib.load()
    if keys.dtype != torch.float32 or keys.dim() != 1 or not keys.is_cuda or not keys.is_contiguous():
        raise ValueError('keys: a contiguous 1-D float32 device tensor')
    n, num = keys.numel(), int(num)
    nbytes = lib.igmc_select_scratch_bytes(n, num, int(grid))
    if nbytes < 0:
        raise RuntimeError('igmc_select_scratch_bytes failed: %s' % lib.cdll.igmc_last_error().decode())
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=keys.device)
    idx = torch.empty(2, num, dtype=torch.int32, device=keys.device)
    key = torch.empty(2, num, dtype=torch.float32, device=keys.device)
    count = torch.zeros(1, dtype=torch.int32, device=keys.device)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    lib.call('igmc_select_extremes', _p(keys.data_ptr()), n, num, _p(idx[0].data_ptr()), _p(idx[1].data_ptr()),
             _p(key[0].data_ptr()), _p(key[1].data_ptr()), _p(count.data_ptr()), _p(scratch.data_ptr()), nbytes, int(grid),
             _p(st))
    c = min(n, num)
    return idx[0, :c], idx[1, :c], key[0, :c], key[1, :c]


def select_segments(keys, seg_off, num, geometry=0, lib=None, stream=None):
    """The ``num`` first of every segment ``[seg_off[s], seg_off[s + 1])`` of a device float32 vector in the order (key
    descending, index ascending, NaNs last) (``igmc_select_segments``; no reference counterpart).  ``seg_off``: device int64
    ``[ns + 1]``.  Returns device tensors ``(idx int32 [ns, num], key float32 [ns, num], count int32 [ns])``: positions in
    ``keys`` (-1 past the count), the keys' own bits (0 past the count); nothing leaves the device."""
    import torch
    lib = lib or _lib.load()
    if keys.dtype != torch.float32 or keys.dim() != 1 or not keys.is_cuda or not keys.is_contiguous():
        raise ValueError('keys: a contiguous 1-D float32 device tensor')
    if seg_off.dtype != torch.int64 or seg_off.dim() != 1 or not seg_off.is_cuda or not seg_off.is_contiguous():
        raise ValueError('seg_off: a contiguous 1-D int64 device tensor')
    ns, num = seg_off.numel() - 1, int(num)
    nbytes = lib.igmc_select_segments_scratch_bytes(ns, num, int(geometry))
    if nbytes < 0:
        raise RuntimeError('igmc_select_segments_scratch_bytes failed: %s' % lib.cdll.igmc_last_error().decode())
    idx = torch.full((ns, num), -1, dtype=torch.int32, device=keys.device)
    key = torch.zeros(ns, num, dtype=torch.float32, device=keys.device)
    count = torch.zeros(ns, dtype=torch.int32, device=keys.device)
    if keys.numel() == 0:          # (every segment is empty: nothing to launch over)
        return idx, key, count
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=keys.device)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    lib.call('igmc_select_segments', _p(keys.data_ptr()), _p(seg_off.data_ptr()), ns, num, _p(idx.data_ptr()),
             _p(key.data_ptr()), _p(count.data_ptr()), _p(scratch.data_ptr()), nbytes, int(geometry), _p(st))
    return idx, key, count


def _must_args(must):
    if must is None:
        return None, None, 0
    return _p(must[0].data_ptr()), _p(must[1].data_ptr() if must[1].numel() else None), must[1].numel()


def _candidates_args(graph, users, mask, exclude_seen, negatives, must):
    """The entry point's prefix (``igmc_candidates`` / ``igmc_candidates_sample``) and the leading arguments its count and its
    fill share."""
    head = (graph.handle, _p(users.data_ptr()), users.numel(), _p(None if mask is None else mask.data_ptr()),
            int(bool(exclude_seen)))
    if negatives is None:
        return 'igmc_candidates', head
    if not 0 <= int(negatives) <= 2 ** 31 - 1:
        raise ValueError('negatives must be in [0, 2^31)')
    return 'igmc_candidates_sample', head + _must_args(must) + (int(negatives),)


def candidates_count(graph, users, mask, exclude_seen, negatives=None, must=None, stream=None):
    """Per-user candidate counts of ``users`` (device int32) over ``graph`` (``igmc_candidates_count``; ``negatives=K``:
    ``igmc_candidates_sample_count`` -- K sampled negatives + the must items, ``must = (offsets int64 [nq + 1], items
    int32)``, device tensors; no reference counterpart).  ``mask``: device uint8 ``[n_items]`` or None.  Returns device
    tensors ``(counts int64 [nq], err int32 [1])``; the error word is left to the caller to read."""
    import torch
    counts = torch.zeros(users.numel(), dtype=torch.int64, device=users.device)
    err = torch.zeros(1, dtype=torch.int32, device=users.device)
    name, args = _candidates_args(graph, users, mask, exclude_seen, negatives, must)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    graph.lib.call(name + '_count', *(args + (_p(counts.data_ptr()), _p(err.data_ptr()), _p(st))))
    return counts, err


def candidates_fill(graph, users, mask, exclude_seen, offsets, link_u, link_v, err, negatives=None, must=None, seed=0,
                    draw=0, forced=None, stream=None):
    """The candidate links of ``users`` written at ``offsets`` (device int64 ``[nq + 1]``: the prefix sums of
    :func:`candidates_count` under the same arguments) into the device int32 buffers ``link_u`` / ``link_v``
    (``igmc_candidates_fill``; ``negatives=K``: ``igmc_candidates_sample_fill`` under ``seed`` / ``draw``, which also marks
    the must items in ``forced``, device uint8 or None).  ``err`` collects the error bits and is left to the caller."""
    import torch
    name, args = _candidates_args(graph, users, mask, exclude_seen, negatives, must)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    out = (_p(offsets.data_ptr()), _p(link_u.data_ptr()), _p(link_v.data_ptr()))
    if negatives is not None:
        args += (int(seed), int(draw))
        out += (_p(None if forced is None else forced.data_ptr()),)
    graph.lib.call(name + '_fill', *(args + out + (link_u.numel(), _p(err.data_ptr()), _p(st))))


HOLD_ALL = 2 ** 63 - 1      # ``hold``: no limit on the entries a split holds out


def _holdout_head(graph, users, keep, hold):
    hold = HOLD_ALL if hold is None else int(hold)
    if int(keep) < 0 or not 0 <= hold <= HOLD_ALL:
        raise ValueError('keep and hold must be at least 0')
    return graph.handle, _p(users.data_ptr()), users.numel(), int(keep), hold


def holdout_count(graph, users, keep, hold=None, stream=None):
    """How many entries the Given-k split holds out of the row of every user of ``users`` (device int32):
    ``min(hold, max(0, d - keep))`` (``igmc_holdout_count``; ``hold=None``: no limit; no reference counterpart).  Returns
    device tensors ``(counts int64 [nq], err int32 [1])``; the error word is left to the caller to read."""
    import torch
    counts = torch.zeros(users.numel(), dtype=torch.int64, device=users.device)
    err = torch.zeros(1, dtype=torch.int32, device=users.device)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    graph.lib.call('igmc_holdout_count', *(_holdout_head(graph, users, keep, hold) + (_p(counts.data_ptr()), _p(err.data_ptr()),
                                                                                      _p(st))))
    return counts, err


def holdout_fill(graph, users, keep, hold, offsets, link_u, link_v, rating, err, seed=0, draw=0, stream=None):
    """The held-out links of ``users`` written at ``offsets`` (device int64 ``[nq + 1]``: the prefix sums of
    :func:`holdout_count` under the same arguments) into the device buffers ``link_u`` / ``link_v`` (int32) and ``rating``
    (uint8: relation + 1), every user's in its row's own order (``igmc_holdout_fill``; ``include/igmc_hip.h`` states the
    definition): per user the ``d - held`` entries with the smallest hash key under ``(seed, draw, user id)`` stay.  ``err``
    collects the error bits and is left to the caller."""
    import torch
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    graph.lib.call('igmc_holdout_fill', *(_holdout_head(graph, users, keep, hold) + (
        int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1), _p(offsets.data_ptr()), _p(link_u.data_ptr()),
        _p(link_v.data_ptr()), _p(rating.data_ptr()), link_u.numel(), _p(err.data_ptr()), _p(st))))


def pair_negatives(graph, pos_u, pos_v, n, mask, seed, epoch, link_u, link_v, link_y, err, stream=None):
    """One negative per positive ``(pos_u[k], pos_v[k])``, ``k < n``, drawn under ``(seed, epoch, k)`` into the ``2 n`` slots of
    ``link_u`` / ``link_v`` / ``link_y`` (``igmc_pair_negatives``; no reference counterpart).  Every argument but the scalars
    is a device address (or None for ``mask``); ``err`` collects the error bits and is left to the caller."""
    graph.lib.call('igmc_pair_negatives', graph.handle, _p(pos_u), _p(pos_v), int(n), _p(mask), int(seed) & (2 ** 64 - 1),
                   int(epoch) & (2 ** 64 - 1), _p(link_u), _p(link_v), _p(link_y), _p(err), _p(stream))


def pair_negatives_shortlist(graph, pos_u, pos_v, n, mask, seed, epoch, sl_off, sl_item, sl_total, hard_share, link_u, link_v,
                             link_y, err, stream=None):
    """:func:`pair_negatives` with a share ``hard_share`` of the negatives asked of a per-user table (``sl_off`` int64
    ``[n_users + 1]``, ``sl_item`` int32 ``[sl_total]``: every user's co-rating shortlist) -- ``igmc_pair_negatives_shortlist``;
    such a negative's label is 2.  ``err`` gains bit 2 (a picked item did not qualify: a stale table) and bit 3 (offsets that
    are no segment of the table)."""
    graph.lib.call('igmc_pair_negatives_shortlist', graph.handle, _p(pos_u), _p(pos_v), int(n), _p(mask),
                   int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1), _p(sl_off), _p(sl_item), int(sl_total), float(hard_share),
                   _p(link_u), _p(link_v), _p(link_y), _p(err), _p(stream))


def pair_kind_stats(lib, out, y, B, stats6, stream=None):
    """Count, ordered pairs and pair-term sum of a pair batch's uniform (label 1) and shortlist (label 2) negatives into the
    device float64 ``[6]`` at ``stats6`` (``igmc_pair_kind_stats``); every argument but ``B`` is a device address."""
    lib.call('igmc_pair_kind_stats', _p(out), _p(y), int(B), _p(stats6), _p(stream))


def _shortlist_scratch(graph, nq, grid, dev):
    """The graph's shortlist scratch (kept on the ``Graph`` and grown on demand) as ``(pointer, bytes)``; ``(None, 0)`` where
    both tables of a workgroup fit its LDS."""
    import torch
    nbytes = graph.lib.igmc_shortlist_scratch_bytes(graph.handle, int(nq), int(grid))
    if nbytes < 0:
        raise RuntimeError('igmc_shortlist_scratch_bytes failed: %s' % graph.lib.cdll.igmc_last_error().decode())
    if nbytes == 0:
        return None, 0
    have = getattr(graph, '_shortlist_scratch', None)
    if have is None or have.numel() * 4 < nbytes or have.device != dev:
        have = graph._shortlist_scratch = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
    return _p(have.data_ptr()), nbytes


def _shortlist_head(graph, users, mask, exclude_seen, seed_min_rel, vote_min_rel):
    if min(int(seed_min_rel), int(vote_min_rel)) < 0:
        raise ValueError('seed_min_rel and vote_min_rel must be at least 0')
    return (graph.handle, _p(users.data_ptr()), users.numel(), _p(None if mask is None else mask.data_ptr()),
            int(bool(exclude_seen)), int(seed_min_rel), int(vote_min_rel))


def shortlist_fill(graph, users, mask, exclude_seen, m, offsets, link_u, link_v, err, votes=None, seed_min_rel=0,
                   vote_min_rel=0, grid=0, stream=None):
    """Every user's ``min(m, candidates)`` candidates with the most co-rating votes, item ascending, written at ``offsets``
    (device int64 ``[nq + 1]``: the prefix sums of :func:`candidates_count` clamped to ``m``) into the device int32 buffers
    ``link_u`` / ``link_v`` and -- ``votes``: device int32 / uint32 of the same length, or None -- their vote counts
    (``igmc_shortlist_fill``; ``include/igmc_hip.h`` states the definition; no reference counterpart).  A user without a
    seeding entry gets its ``m`` lowest candidate ids.  ``err`` collects the error bits of :func:`candidates_fill` and is
    left to the caller."""
    import torch
    if not 1 <= int(m) <= 2 ** 31 - 1:
        raise ValueError('shortlist size must be in [1, 2^31)')
    head = _shortlist_head(graph, users, mask, exclude_seen, seed_min_rel, vote_min_rel)
    sp, sb = _shortlist_scratch(graph, users.numel(), grid, users.device)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    graph.lib.call('igmc_shortlist_fill', *(head + (int(m), _p(offsets.data_ptr()), _p(link_u.data_ptr()), _p(link_v.data_ptr()),
                                                    _p(None if votes is None else votes.data_ptr()), link_u.numel(),
                                                    _p(err.data_ptr()), sp, sb, int(grid), _p(st))))


def shortlist_places(graph, users, mask, exclude_seen, q_off, q_id, seed_min_rel=0, vote_min_rel=0, err=None, grid=0,
                     stream=None):
    """Where the items ``q_id`` (device int32; request ``q`` owns ``q_id[q_off[q]:q_off[q + 1]]``, ``q_off`` device int64
    ``[nq + 1]``) stand in the FULL vote order of their users (``igmc_shortlist_places``).  Returns device tensors ``(place
    int32, votes int32)``: the number of candidates before the item (votes descending, item id ascending) or -1 where it is no
    candidate, and its vote count (below 2^31 by the entry point's own limit).  "In the shortlist of size m" is ``0 <= place <
    m``.  ``err``: as in :func:`rank_segments` (bit 0: inconsistent ``q_off``; bit 1: a user id out of range)."""
    import torch
    _dev_vector(q_off, torch.int64, 'q_off')
    _dev_vector(q_id, torch.int32, 'q_id')
    if q_off.numel() != users.numel() + 1:
        raise ValueError('one query range per requested user')
    nquery = q_id.numel()
    place = torch.full((nquery,), -1, dtype=torch.int32, device=users.device)
    votes = torch.zeros(nquery, dtype=torch.int32, device=users.device)
    if nquery == 0:
        return place, votes
    own = err is None
    if own:
        err = torch.zeros(1, dtype=torch.int32, device=users.device)
    head = _shortlist_head(graph, users, mask, exclude_seen, seed_min_rel, vote_min_rel)
    sp, sb = _shortlist_scratch(graph, users.numel(), grid, users.device)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    graph.lib.call('igmc_shortlist_places', *(head + (_p(q_off.data_ptr()), _p(q_id.data_ptr()), nquery, _p(place.data_ptr()),
                                                      _p(votes.data_ptr()), _p(err.data_ptr()), sp, sb, int(grid), _p(st))))
    if own:
        e = int(err.item())
        if e:
            raise RuntimeError('igmc_shortlist_places: %s (err=%d)' % (
                '; '.join(w for b, w in ((1, RANK_ERRORS[0][1]), (2, 'a user id outside [0, n_users)')) if e & b), e))
    return place, votes


RANK_ERRORS = ((1,'query offsets that are not 0 = q_off[0] <= ... <= q_off[ns] = the number of queries'),
               (2, 'a segment outside the keys'))


def _dev_vector(t, dtype, what):
    if t.dtype != dtype or t.dim() != 1 or not t.is_cuda or not t.is_contiguous():
        raise ValueError('%s: a contiguous 1-D %s device tensor' % (what, str(dtype).replace('torch.', '')))


def rank_segments(keys, ids, seg_off, q_off, q_id, geometry=0, err=None, lib=None, stream=None):
    """Where the ids ``q_id`` stand in their segments (``igmc_rank_segments``; no reference counterpart).  ``keys`` float32 /
    ``ids`` int32 ``[n]`` (ids strictly ascending inside every segment), ``seg_off`` / ``q_off`` int64 ``[ns + 1]``: segment
    ``s`` owns the queries ``q_id[q_off[s]:q_off[s + 1]]`` (int32).  Returns device tensors ``(pos, rank)`` int32 ``[nq]``:
    the position in ``keys`` of the entry with the query's id and its 0-based place in the order of
    :func:`select_segments` (key descending, index ascending, NaNs last); -1 / -1 where the segment has no such entry.
    ``err``: a zeroed int32 device word that collects the error bits (``RANK_ERRORS``) and is left to the caller to read;
    without it the word is read here (one synchronisation) and a set bit raises.  Nothing else leaves the device."""
    import torch
    lib = lib or _lib.load()
    _dev_vector(keys, torch.float32, 'keys')
    _dev_vector(ids, torch.int32, 'ids')
    _dev_vector(seg_off, torch.int64, 'seg_off')
    _dev_vector(q_off, torch.int64, 'q_off')
    _dev_vector(q_id, torch.int32, 'q_id')
    if ids.numel() != keys.numel() or q_off.numel() != seg_off.numel():
        raise ValueError('one id per key and one query range per segment')
    ns, n, nq = seg_off.numel() - 1, keys.numel(), q_id.numel()
    pos = torch.full((nq,), -1, dtype=torch.int32, device=keys.device)
    rank = torch.full((nq,), -1, dtype=torch.int32, device=keys.device)
    if n == 0 or nq == 0:          # (every segment is empty, or nobody asks: nothing to launch over)
        return pos, rank
    own = err is None
    if own:
        err = torch.zeros(1, dtype=torch.int32, device=keys.device)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    lib.call('igmc_rank_segments', _p(keys.data_ptr()), _p(ids.data_ptr()), n, _p(seg_off.data_ptr()), ns,
             _p(q_off.data_ptr()), _p(q_id.data_ptr()), nq, _p(pos.data_ptr()), _p(rank.data_ptr()), _p(err.data_ptr()),
             int(geometry), _p(st))
    if own:
        _raise_rank_errors(err, 'igmc_rank_segments')
    return pos, rank


def rank_metrics(rank, q_off, ks, relevant=None, grid=0, err=None, lib=None, stream=None):
    """Per-segment sums of the ranking metrics over the ranks of :func:`rank_segments` (``igmc_rank_metrics``; binary
    relevance: a query counts when ``relevant`` -- uint8 ``[nq]``, None = all -- is set and its rank is >= 0).  ``ks``: 1 to 8
    cut-offs K >= 1.  Returns device tensors ``(cnt int32 [ns, 2 + nk], dcg float64 [ns, 2 * nk])``: ``cnt[:, 0]`` = n_rel,
    ``cnt[:, 1]`` = the smallest rank (-1: none), ``cnt[:, 2 + j]`` = #{rank < ks[j]}; ``dcg[:, j]`` = the sum of
    1 / log2(rank + 2) over those, ``dcg[:, nk + j]`` = the same sum for the ideal list of min(K, n_rel) places.  Bit-identical
    for every ``grid``.  ``err``: as in :func:`rank_segments`."""
    import torch
    lib = lib or _lib.load()
    _dev_vector(rank, torch.int32, 'rank')
    _dev_vector(q_off, torch.int64, 'q_off')
    if relevant is not None:
        _dev_vector(relevant, torch.uint8, 'relevant')
        if relevant.numel() != rank.numel():
            raise ValueError('one relevance flag per query')
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= 8 or min(ks) < 1 or max(ks) > 2 ** 31 - 1:
        raise ValueError('ks: 1 to 8 cut-offs K in [1, 2^31)')
    ns, nk = q_off.numel() - 1, len(ks)
    d_ks = torch.tensor(ks, dtype=torch.int32, device=rank.device)
    cnt = torch.zeros(ns, 2 + nk, dtype=torch.int32, device=rank.device)
    dcg = torch.zeros(ns, 2 * nk, dtype=torch.float64, device=rank.device)
    own = err is None
    if own:
        err = torch.zeros(1, dtype=torch.int32, device=rank.device)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    lib.call('igmc_rank_metrics', _p(rank.data_ptr() if rank.numel() else None), _p(q_off.data_ptr()),
             _p(None if relevant is None else relevant.data_ptr()), rank.numel(), ns, _p(d_ks.data_ptr()), nk,
             _p(cnt.data_ptr()), _p(dcg.data_ptr()), _p(err.data_ptr()), int(grid), _p(st))
    if own:
        _raise_rank_errors(err, 'igmc_rank_metrics')
    return cnt, dcg


def _raise_rank_errors(err, what):
    e = int(err.item())
    if e:
        raise RuntimeError('%s: %s (err=%d)' % (what, '; '.join(w for b, w in RANK_ERRORS if e & b), e))


def profile_enable(lib, on):
    lib.igmc_profile_enable(int(bool(on)))


def profile_fetch(lib, cap=64):
    names = ((C.c_char * 48) * cap)()
    ms = (C.c_float * cap)()
    calls = (C.c_int * cap)()
    n = lib.igmc_profile_fetch(C.cast(names, C.c_void_p), C.cast(ms, C.c_void_p), C.cast(calls, C.c_void_p), cap)
    return [(names[i].value.decode(), float(ms[i]), int(calls[i])) for i in range(max(n, 0))]


class SortPoolWorkspace(object):
    """Sort-pool readout (DGCNN_RS, reference ``models.py:63-167``) on top of a :class:`ModelWorkspace`'s conv kernels."""

    KEYS = ['convs.%d.%s' % (l, k) for l in range(4) for k in ('basis', 'root', 'bias', 'att')] + [
        'conv1d_params1.weight', 'conv1d_params1.bias', 'conv1d_params2.weight', 'conv1d_params2.bias',
        'lin1.weight', 'lin1.bias', 'lin2.weight', 'lin2.bias']

    def __init__(self, ws, k, max_nodes_per_graph):
        self.ws, self.lib = ws, ws.lib
        h = C.c_void_p()
        self.lib.call('igmc_sortpool_create', ws.handle, int(k), int(max_nodes_per_graph), C.byref(h))
        self.handle = h
        lay = (C.c_int64 * 27)()
        self.lib.call('igmc_sortpool_layout', h, C.cast(lay, C.c_void_p))
        self.offsets = dict(zip(self.KEYS, [int(x) for x in lay[:24]]))
        self.n_params, self.dense, self.k = int(lay[24]), int(lay[25]), int(lay[26])

    def __del__(self):
        try:
            self.lib.cdll.igmc_sortpool_destroy(self.handle)
        except Exception:
            pass

    def forward(self, params, batch, out, training=False, use_edge_flags=False, lin_mask=None, seed=0, step=0, stream=None):
        self.lib.call('igmc_sortpool_forward', self.handle, _p(params), batch.handle, int(bool(training)),
                      int(bool(use_edge_flags)), _p(lin_mask), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1),
                      _p(out), _p(stream))

    def loss_grad(self, params, batch, out, grad, loss, use_edge_flags=False, lin_mask=None, seed=0, step=0, ARR=0.0,
                  grad_scale=None, arr_scale=1.0, stream=None):
        if grad_scale is None:
            grad_scale = 1.0 / batch.B
        self.lib.call('igmc_sortpool_loss_grad', self.handle, _p(params), batch.handle, int(bool(use_edge_flags)),
                      _p(lin_mask), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), float(ARR), float(grad_scale),
                      float(arr_scale), _p(out), _p(grad), _p(loss), _p(stream))
