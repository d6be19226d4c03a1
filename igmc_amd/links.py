"""What "dataset-shaped" means here, written once: :class:`LinkSource` is what ``stepgraph.StepGraph`` / ``ScoreGraph``,
``train_eval.score_links`` / ``DataLoader`` and ``IGMC._workspace`` read of the object they are given -- a list of links over a
device-resident rating graph whose enclosing subgraphs are extracted into engine arenas.  The datasets of
``util_functions``, ``recommend.CandidateLinks`` and ``explain.LeaveOneOutLinks`` derive from it and add only what is theirs.
"""
import numpy as np
import torch

from . import engine


class DeviceBatch(object):
    """One extracted + collated batch living in an engine arena (valid until the arena is reused).

    Carries what ``IGMC.forward`` / the train loop need (``num_graphs``, ``y``) and materialises the
    PyG-style tensors (``x, edge_index, edge_type, batch``) lazily on request (host round trip; only for
    inspection / compatibility -- the model consumes the arena directly)."""

    def __init__(self, dataset, arena, num_graphs, positions, first, side=None):
        self.dataset = dataset
        self.arena = arena
        self.num_graphs = int(num_graphs)
        self._positions, self._first = positions, int(first)
        self.side = side            # [B, n_side] device tensor or None
        self._pyg = None
        self._y = None

    @property
    def link_pos(self):
        """Dataset positions of the batch's links (device int64)."""
        if self._positions is None:
            return torch.arange(self._first, self._first + self.num_graphs, device=self.dataset.link_y.device)
        return self._positions[self._first:self._first + self.num_graphs].long()

    @property
    def y(self):
        """Rating values of the batch (lazy: the kernels read them straight from the dataset's link array)."""
        if self._y is None:
            self._y = self.dataset.link_y.index_select(0, self.link_pos)
        return self._y

    def to(self, device):
        return self

    def _materialise(self):
        if self._pyg is None:
            d = self.arena.download(torch.cuda.current_stream().cuda_stream)
            N = d['N']
            dst = np.repeat(np.arange(N, dtype=np.int64), np.diff(d['row_ptr']).astype(np.int64))
            x = np.zeros((N, self.arena.num_labels), np.float32)
            x[np.arange(N), d['node_label']] = 1.0
            self._pyg = dict(x=torch.from_numpy(x), edge_index=torch.from_numpy(np.stack([d['col'].astype(np.int64), dst], 0)),
                             edge_type=torch.from_numpy(d['erel'].astype(np.int64)),
                             batch=torch.from_numpy(d['node_graph'].astype(np.int64)), raw=d)
        return self._pyg

    x = property(lambda self: self._materialise()['x'])
    edge_index = property(lambda self: self._materialise()['edge_index'])
    edge_type = property(lambda self: self._materialise()['edge_type'])
    batch = property(lambda self: self._materialise()['batch'])


class _DevRows(object):
    """``[rows, cols]`` float32 values at a device address, for ``torch.as_tensor`` (no copy)."""

    def __init__(self, ptr, rows, cols):
        self.__cuda_array_interface__ = dict(shape=(int(rows), int(cols)), typestr='<f4', data=(int(ptr), False), version=2)


def refuse_side_features(source):
    """A source that names side features but cannot hand out per-node tables (``node_side()``) is refused: links that are not
    its own would silently be scored without their feature rows."""
    if getattr(source, '_side', None) is not None or getattr(source, 'u_features', None) is not None or \
            getattr(source, 'v_features', None) is not None:
        raise NotImplementedError('this source names side features (--use-features: u_features / v_features) but has no '
                                  'node_side() tables to gather them from by node id: serve from a dataset of '
                                  'util_functions, or from a view of one')


def dense_side_table(features, what, rows=None, cols=None):
    """``features`` (scipy sparse or array, one row per node) as a dense contiguous float32 host array; ``rows`` / ``cols``:
    the least row count / the exact column count it must have (``ValueError``)."""
    f = features.toarray() if hasattr(features, 'toarray') else np.asarray(features)
    if f.ndim != 2:
        raise ValueError('%s: one feature row per node' % what)
    if rows is not None and f.shape[0] < rows:
        raise ValueError('%s: %d rows, at least %d expected' % (what, f.shape[0], rows))
    if cols is not None and f.shape[1] != cols:
        raise ValueError('%s: %d columns, %d expected' % (what, f.shape[1], cols))
    return np.ascontiguousarray(f, dtype=np.float32)


class LinkSource(object):
    """Links over a rating graph in HBM, and how a batch of them gets into an arena.

    SETTINGS (:meth:`_configure`, or :meth:`_configure_from` another source or view): ``graph``, ``lib``, ``device``, ``h``,
    ``sample_ratio``, ``seed``, ``max_nodes_per_hop``; ``dynamic`` -- the sampler takes the epoch it is given (False: always
    epoch 0, the same subgraphs every pass).

    STORAGE, device tensors a subclass allocates ONCE (captured launches hold their addresses): ``link_y`` float32, one label
    per position, always; ``link_u`` / ``link_v`` int32 where the subgraphs are extracted from the graph; where they are
    rebuilt from stored node sets instead, ``_cache_t`` -- the six tensors ``uoff voff unodes vnodes udist vdist`` -- and
    ``_cache``, their device pointers (``None``: no cache); side features of the target nodes: ``_side`` float32 ``[capacity,
    n_side_features]``, their rows per position (a dataset's own links; where set, batches gather from it), else
    ``_side_tables`` = ``(U [n_u, fu], V [n_v, fv])`` float32, one row per node, gathered by the ids of a batch's targets (links
    that are nobody's own: candidate lists, leave-one-out variants, views); both ``None``: no side features.

    ``capacity`` is the number of positions ``link_y`` holds: what everything that keeps a buffer per position
    (``ScoreGraph``'s scores and labels, ``StepGraph``'s permutation) is sized by.  ``len()`` is the number of links held NOW; a
    source that is refilled in place overrides it, every other one is full."""
    dynamic = True
    link_u = link_v = None
    _cache = _cache_t = None
    _side, _side_tables, n_side_features = None, None, 0

    def _configure(self, graph, device, h, sample_ratio, seed, max_nodes_per_hop):
        self.graph, self.lib, self.device = graph, graph.lib, device
        self.h, self.sample_ratio, self.seed = int(h), float(sample_ratio), int(seed)
        self.max_nodes_per_hop = None if max_nodes_per_hop is None else int(max_nodes_per_hop)
        self._arenas = {}

    def _configure_from(self, source, graph=None):
        """The settings of ``source`` (a dataset, or a view of one over another graph), over ``graph`` where given, and its
        per-node side-feature tables where it has them (``node_side()``: the SAME tensors, so every source derived from a
        dataset gathers from one copy).  A source that names side features without such tables is refused."""
        tables = source.node_side() if hasattr(source, 'node_side') else None
        if tables is None:
            refuse_side_features(source)
        self.source = source
        self._configure(source.graph if graph is None else graph, source.device, source.h, source.sample_ratio, source.seed,
                        source.max_nodes_per_hop)
        self._take_side_tables(tables)

    def _take_side_tables(self, tables):
        self._side_tables = tables
        self.n_side_features = 0 if tables is None else tables[0].shape[1] + tables[1].shape[1]

    def node_side(self):
        """``(U [n_u, fu], V [n_v, fv])``: the per-node side-feature tables this source serves with -- dense float32 device
        tensors allocated once (captured launches hold their addresses) --, or None."""
        return self._side_tables

    def __len__(self):
        return self.capacity

    @property
    def capacity(self):
        return self.link_y.numel()

    @property
    def num_features(self):
        return 2 * self.h + 2          # one-hot of the node label (reference util_functions.py:246, :285)

    @property
    def group_extractable(self):
        """A group's batches can go into their arenas in one launch per stage (``engine.BatchSet``: ``link_u`` / ``link_v``,
        nothing else to gather)."""
        return self._cache is None and self._side is None and self._side_tables is None

    def arena(self, max_graphs, slot=0):
        key = (int(max_graphs), slot)
        if key not in self._arenas:
            a = engine.Batch(self.graph, int(max_graphs), self.h, self.max_nodes_per_hop)
            # the target nodes' feature rows are gathered by the extraction launch itself (device-side, also under hipGraph
            # replay of the training step): by link position from a dataset's own matrix, by target id from node tables
            if self._side is not None:
                a.bind_side_source(self._side.data_ptr(), self.n_side_features)
            elif self._side_tables is not None:
                U, V = self._side_tables
                a.bind_side_tables(U.data_ptr(), U.shape[0], U.shape[1], V.data_ptr(), V.shape[0], V.shape[1])
            self._arenas[key] = a
        return self._arenas[key]

    def extract_into(self, arena, positions_ptr, first, B, epoch=0, stream=None):
        """Links ``positions[first:first+B]`` (address of a device int32 array, or None = identity; under the device-side step
        control ``first`` selects the batch instead) into ``arena``: rebuilt from the node-set cache where there is one,
        else extracted from the graph under the sampling key (seed, epoch, position)."""
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        if self._cache is not None:
            arena.extract_cached(self._cache, self.link_y.data_ptr(), positions_ptr, first, B, st)
        else:
            arena.extract(self.link_u.data_ptr(), self.link_v.data_ptr(), self.link_y.data_ptr(), positions_ptr, first, B,
                          self.sample_ratio, self.seed, epoch if self.dynamic else 0, st)

    def extract(self, positions, first, B, epoch=0, slot=0, max_graphs=None, stream=None):
        """Extract links ``positions[first:first+B]`` (device int32 tensor, or None = identity) into an arena."""
        arena = self.arena(max_graphs or B, slot)
        self.extract_into(arena, None if positions is None else positions.data_ptr(), first, B, epoch, stream)
        db = DeviceBatch(self, arena, B, positions, first)
        if self._side is not None:        # view of the rows the extraction launch gathered (for inspection / get())
            db.side = self._side.index_select(0, db.link_pos)
        elif self._side_tables is not None:        # a copy of the arena's own gathered rows, taken behind the gather on `stream`
            with torch.cuda.stream(torch.cuda.current_stream() if stream is None else torch.cuda.ExternalStream(int(stream))):
                db.side = torch.as_tensor(_DevRows(arena.device_ptr('SIDE'), B, self.n_side_features),
                                          device=self.link_y.device).clone()
        return db


def kept(dataset, name, fits, make):
    """The object a serving stage keeps as ``dataset.<name>`` so that its passes replay what the first one captured: the kept
    one where it was built over this dataset and its graph and ``fits(obj)``, else ``make()``, kept from now on."""
    obj = getattr(dataset, name, None)
    if obj is None or obj.source is not dataset or obj.graph is not dataset.graph or not fits(obj):
        obj = make()
        setattr(dataset, name, obj)
    return obj
