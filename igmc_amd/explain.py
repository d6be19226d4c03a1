"""Why a prediction: leave-one-out neighbour attribution on the device (no reference counterpart: the reference's
``visualize`` draws an enclosing subgraph and leaves the reading to the eye).

An IGMC prediction is a function of one enclosing subgraph and nothing else, so its "reason" is concrete: which neighbours
in that subgraph -- the items this user rated, the users who rated this item -- move the score, and by how much.

DEFINITION.  Take a link (u, v), extracted under the scoring key (``SCORE_EPOCH``, position = its index in the list given to
:func:`explain`, exactly as ``recommend.score_candidates`` over ``CandidateLinks.from_pairs`` sees it).  Its node set is users
``U[0..nu)`` and items ``V[0..nv)`` in slot order: the target first on each side, the rest by ascending id, every node with its
hop distance.  Its VARIANTS are, in this order, the whole set (the base), the set without ``U[j]`` for j = 1 .. nu-1, the set
without ``V[j]`` for j = 1 .. nv-1.  The two targets are never removed.  Every remaining node keeps the hop distance -- and so
the label -- it had in the whole subgraph: AT HOP 2 A NODE REACHABLE ONLY THROUGH THE REMOVED ONE STAYS, WITH ITS OLD LABEL.
Each variant is scored by the ordinary cached-extraction path (``igmc_extract_batch_cached``: the edges induced among the
remaining nodes, without the target edge, then the forward pass), and

    delta(link, node) = score(variant without node) - score(base variant).

A link whose targets have no neighbours has the base variant only and an empty attribution segment.  Removal, not masking: an
isolated node would still take part in ``DGCNN_RS``'s sort-pool, and removal needs no new arena state.

HOW (``igmc_amd/csrc/explain.hip``).  The pairs are extracted in batches through a ``CandidateLinks.from_pairs`` arena;
``igmc_loo_count`` sizes every link's variants from the arena, ``igmc_loo_fill`` writes them -- straight from the arena's
slots -- into the node-set cache of a :class:`LeaveOneOutLinks`, ``score_links`` scores that ``links.LinkSource`` like any
static dataset (a captured ``ScoreGraph``, sized by its ``capacity``, is replayed by every later pass), ``igmc_loo_deltas`` turns the scores into
contiguous attribution segments and ``igmc_select_segments`` takes the ``m`` largest ``|delta|`` of each.  Per pass ONE host
read -- the three totals of the counts -- crosses to the host; the error words are read once per call.

SAMPLER POSITIONS.  As ``recommend.py`` says of its candidates: the extraction's sampler is keyed by (seed, epoch, link
position).  Where a per-hop cap binds, the sampled subgraph of a pair -- hence its base score and its attributions -- depends on
the pair's POSITION IN THE LIST given to :func:`explain`; every result is a deterministic function of (seed, the list).  The
position is the index in the whole list, not in a pass, and the variants are replayed from the cache without any draw, so the
results do not depend on ``links_per_pass``, with or without a binding cap.
"""
import numpy as np
import torch

from . import engine
from .links import LinkSource, kept
from .recommend import CandidateLinks, score_candidates

# Capacities of a LeaveOneOutLinks where the caller names none.  A link with nu users and nv items has nu + nv - 1 variants
# holding nu + (nu-1)^2 + (nv-1) nu user entries and nv + (nu-1) nv + (nv-1)^2 item entries.  At the headline shape (one hop,
# max_nodes_per_hop = 100: at most 101 + 101 nodes) that is at most 201 variants and 20 201 entries a side per link, so
# 2^16 variants hold 326 such links and 2^23 entries a side 415 of them: a few hundred links per pass.  The buffers take
# 2 * 2^23 * (4 + 1) bytes = 84 MB for the node lists, 1 MB of offsets and 0.7 MB of per-variant arrays.
DEFAULT_VARIANTS = 1 << 16
DEFAULT_ENTRIES = 1 << 23

_ERRORS = ((1, 'a link\'s variants reach past the variant capacity'),
           (2, 'a link\'s user entries reach past the entry capacity'),
           (4, 'a link\'s item entries reach past the entry capacity'),
           (8, 'offsets that are not the prefix sums of the counts'),
           (16, 'an arena slot without an extracted link'))


class LeaveOneOutLinks(LinkSource):
    """The leave-one-out variants of a pass of links as a STATIC source (``dynamic = False``, a ``_cache`` of node sets in
    HBM): a ``links.LinkSource`` with the settings of ``dataset_or_view`` and a ``link_y`` of zeros, whose batches are rebuilt
    from the cache (nothing is sampled, the epoch does not matter).

    The six cache tensors and the per-variant arrays have FIXED ADDRESSES AND CAPACITIES and are refilled in place by every
    pass, so the hipGraph a scoring pass captured is replayed by the later ones.  ``len()`` is the number of variants the
    last pass wrote, ``capacity`` (= ``capacity_variants``) the number they have room for.  ``dataset_or_view``: a dataset or a
    ``recommend.GraphView``; with side features, every variant gathers the rows of its two targets -- its base link's -- from
    the source's per-node tables."""
    dynamic = False

    def __init__(self, dataset_or_view, capacity_variants=DEFAULT_VARIANTS, capacity_entries=DEFAULT_ENTRIES):
        self._configure_from(dataset_or_view)
        cv, ce = int(capacity_variants), int(capacity_entries)
        if not 1 <= cv <= 2 ** 31 - 1 or ce < 1:
            raise ValueError('capacity_variants must be in [1, 2^31) and capacity_entries at least 1')
        self.capacity_variants, self.capacity_entries = cv, ce
        dev = dataset_or_view.link_y.device
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
        # A replayed launch prefetches past the end of a short pass (as CandidateLinks' zero-initialised link buffers say):
        # positions behind the last variant must describe valid node sets.  Every pass points the unused tail of uoff / voff
        # at one-entry sets BEHIND its own entries (_close_tail), so the node arrays carry capacity_variants + 1 entries more
        # than the capacity the kernels may fill; whatever those entries hold -- zeros, or ids an earlier pass wrote -- is a
        # valid id with a valid distance.
        self._cache_t = dict(uoff=z(cv + 1, torch.int64), voff=z(cv + 1, torch.int64),
                             unodes=z(ce + cv + 1, torch.int32), vnodes=z(ce + cv + 1, torch.int32),
                             udist=z(ce + cv + 1, torch.uint8), vdist=z(ce + cv + 1, torch.uint8))
        self._cache = {k: t.data_ptr() for k, t in self._cache_t.items()}
        self.link_y = z(cv, torch.float32)
        self.var_link, self.var_node = z(cv, torch.int32), z(cv, torch.int32)
        self.var_side, self.var_rating = z(cv, torch.uint8), z(cv, torch.uint8)
        self._ramp = torch.arange(cv + 1, dtype=torch.int64, device=dev)
        self.n = 0
        self._close_tail(0, 0, 0)

    def _close_tail(self, n_variants, n_uent, n_vent):
        """Positions n_variants .. capacity: sets of one user and one item (see the constructor)."""
        self.n = int(n_variants)
        k = self.capacity - self.n
        self._cache_t['uoff'][self.n:] = self._ramp[:k + 1] + int(n_uent)
        self._cache_t['voff'][self.n:] = self._ramp[:k + 1] + int(n_vent)

    def __len__(self):
        return self.n


def _pass_plan(cands, loo, n, batch_size, links_per_pass):
    """Links per pass: by default the largest number whose WORST CASE fits the capacities -- a link of an arena with ``s``
    slots a subgraph has at most s - 1 variants and fewer than (s - 1)^2 entries a side --, at least one."""
    if links_per_pass is not None:
        return max(1, min(int(links_per_pass), n))
    a = cands.arena(batch_size, slot=('explain', 0))
    s = max(2, a.node_capacity // a.max_graphs)
    return max(1, min(n, loo.capacity_variants // (s - 1), loo.capacity_entries // ((s - 1) * (s - 1))))


def _variant_passes(model, dataset, u, v, batch_size, links_per_pass, capacity_variants, capacity_entries, stats):
    """The pass loop: a generator of ``(l0, L, loo, offs, scores)`` -- the pass's first link and number of links, the ONE
    :class:`LeaveOneOutLinks` every pass refills (kept as ``dataset._explain_links``), the int64 ``[3, L + 1]`` prefix sums
    of (variants, user entries, item entries) and one score per variant."""
    from . import train_eval
    if model.flat_parameters().device.type != train_eval.device.type:
        model.to(train_eval.device)
    B = int(batch_size)
    cands = kept(dataset, '_explain_pairs', lambda c: c.capacity >= len(u), lambda: CandidateLinks(dataset, max(1, len(u))))
    cands.set_pairs(u, v)                                     # (ValueError for a pair outside the graph)
    n = len(cands)
    if n < 1:
        raise ValueError('no links to explain')
    dev = cands.link_y.device
    cv = DEFAULT_VARIANTS if capacity_variants is None else int(capacity_variants)
    ce = DEFAULT_ENTRIES if capacity_entries is None else int(capacity_entries)
    loo = kept(dataset, '_explain_links',          # (a capacity the caller does not name: whatever the kept one has)
               lambda o: (capacity_variants is None or o.capacity_variants == cv) and
                         (capacity_entries is None or o.capacity_entries == ce),
               lambda: LeaveOneOutLinks(dataset, cv, ce))
    lpp = _pass_plan(cands, loo, n, B, links_per_pass)
    lib, P = loo.lib, engine._p
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    t = loo._cache_t
    n_var, n_pass = 0, 0
    for l0 in range(0, n, lpp):
        L = min(lpp, n - l0)
        st = torch.cuda.current_stream().cuda_stream
        counts = torch.zeros(3, L, dtype=torch.int64, device=dev)
        arenas = []
        for i, b0 in enumerate(range(0, L, B)):
            Bi = min(B, L - b0)
            a = cands.arena(B, slot=('explain', i))
            a.set_lean(True)          # (only the node slots are read: an arena with dense blocks need not emit its CSR)
            cands.extract(None, l0 + b0, Bi, epoch=train_eval.SCORE_EPOCH, slot=('explain', i), max_graphs=B)
            lib.call('igmc_loo_count', a.handle, Bi, P(counts[0, b0:].data_ptr()), P(counts[1, b0:].data_ptr()),
                     P(counts[2, b0:].data_ptr()), P(st))
            arenas.append((a, b0, Bi))
        offs = torch.zeros(3, L + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 1, out=offs[:, 1:])
        nv_, nue, nve = (int(x) for x in offs[:, -1].tolist())          # THE host read of the pass
        if nv_ > loo.capacity_variants or max(nue, nve) > loo.capacity_entries:
            raise ValueError('links %d .. %d have %d variants with %d / %d user / item entries: they do not fit the capacities '
                             '(%d variants, %d entries); lower links_per_pass or raise the capacities' % (
                                 l0, l0 + L - 1, nv_, nue, nve, loo.capacity_variants, loo.capacity_entries))
        for a, b0, Bi in arenas:
            lib.call('igmc_loo_fill', loo.graph.handle, a.handle, Bi, l0 + b0, P(offs[0, b0:].data_ptr()),
                     P(offs[1, b0:].data_ptr()), P(offs[2, b0:].data_ptr()), loo.capacity_variants, loo.capacity_entries,
                     loo.capacity_entries, P(t['uoff'].data_ptr()), P(t['unodes'].data_ptr()), P(t['udist'].data_ptr()),
                     P(t['voff'].data_ptr()), P(t['vnodes'].data_ptr()), P(t['vdist'].data_ptr()), P(loo.var_link.data_ptr()),
                     P(loo.var_side.data_ptr()), P(loo.var_node.data_ptr()), P(loo.var_rating.data_ptr()),
                     P(err.data_ptr()), P(st))
        loo._close_tail(nv_, nue, nve)
        scores = score_candidates(model, loo, B)
        n_var += nv_
        n_pass += 1
        yield l0, L, loo, offs, scores
    e = int(err.item())
    if e:
        raise RuntimeError('leave-one-out variants: %s (err=%d)' % ('; '.join(w for b, w in _ERRORS if e & b), e))
    if stats is not None:
        stats.update(links=n, variants=n_var, attributions=n_var - n, passes=n_pass)


def _deltas(loo, offs, scores, L):
    """(base [L], delta, key [variants - L], seg_off [L + 1]) of a pass (``igmc_loo_deltas``)."""
    dev = scores.device
    seg_off = (offs[0] - torch.arange(L + 1, dtype=torch.int64, device=dev)).contiguous()
    nd = scores.numel() - L
    base = torch.zeros(L, dtype=torch.float32, device=dev)
    delta = torch.zeros(max(nd, 1), dtype=torch.float32, device=dev)
    key = torch.zeros(max(nd, 1), dtype=torch.float32, device=dev)
    P = engine._p
    loo.lib.call('igmc_loo_deltas', P(scores.data_ptr()), P(offs[0].data_ptr()), L, P(base.data_ptr()), P(delta.data_ptr()),
                 P(key.data_ptr()), P(seg_off.data_ptr()), P(torch.cuda.current_stream().cuda_stream))
    return base, delta[:nd], key[:nd], seg_off


def explain(model, dataset, u, v, m=5, batch_size=50, links_per_pass=None, stats=None, capacity_variants=None,
            capacity_entries=None):
    """The ``m`` neighbours that move the prediction of every pair ``(u[i], v[i])`` most (see the module docstring for the
    definition).  ``u`` / ``v``: integer ids, host or device; ``dataset``: a dataset (normally the training set) or a
    ``recommend.GraphView`` -- its rating graph and extraction settings are used.  Returns a dict of device tensors, rows in
    the order of the pairs:

    * ``base`` float32 ``[n]``: the prediction itself (the base variant's score);
    * ``nodes`` int32 ``[n, m]``: global ids of the removed neighbours, -1 behind a link's count;
    * ``sides`` uint8 ``[n, m]``: 0 = a user (someone who rated the item), 1 = an item (something the user rated); 255 padded;
    * ``ratings`` uint8 ``[n, m]``: rating label + 1 of the entry that joins the neighbour to the opposite target in the
      rating graph, 0 if they share none (two hops) and behind the count;
    * ``deltas`` float32 ``[n, m]``: score without the neighbour - base, 0 padded;
    * ``counts`` int32 ``[n]``: min(m, the link's neighbours).

    Order within a link: ``|delta|`` descending; among equal ``|delta|`` users before items and lower ids first; NaNs last
    (``igmc_select_segments``).  ``m=None``: every neighbour, :func:`explain_all`.  The links are divided into passes of
    ``links_per_pass`` (default: what fits the capacities of the :class:`LeaveOneOutLinks`, kept as
    ``dataset._explain_links``); the results do not depend on it.  Where a per-hop cap binds they depend on the pair's
    position in ``u`` / ``v`` (module docstring: SAMPLER POSITIONS).  Works for ``DGCNN_RS`` too (``score_links``' eager
    path).  ``stats``: a dict that receives ``links``, ``variants``, ``attributions`` and ``passes``."""
    if m is None:
        return explain_all(model, dataset, u, v, batch_size, links_per_pass, stats, capacity_variants, capacity_entries)
    m = int(m)
    if not 1 <= m <= 64:
        raise ValueError('m must be in [1, 64]')
    out = dict(base=[], nodes=[], sides=[], ratings=[], deltas=[], counts=[])
    for l0, L, loo, offs, scores in _variant_passes(model, dataset, u, v, batch_size, links_per_pass, capacity_variants,
                                                    capacity_entries, stats):
        base, delta, key, seg_off = _deltas(loo, offs, scores, L)
        idx, _, count = engine.select_segments(key, seg_off, m, lib=loo.lib)
        have = idx >= 0
        at = idx.clamp(min=0).long()
        # attribution a of link i is variant a + i + 1 of the pass: seg_off[i] = var_off[i] - i, the bases dropped out
        var = (at + torch.arange(1, L + 1, device=idx.device).unsqueeze(1)).clamp(max=len(loo) - 1)
        pick = lambda src, pad: torch.where(have, src[:len(loo)][var], torch.full_like(idx, pad, dtype=src.dtype))
        out['base'].append(base)
        out['nodes'].append(pick(loo.var_node, -1))
        out['sides'].append(pick(loo.var_side, 255))
        out['ratings'].append(pick(loo.var_rating, 0))
        padded = torch.cat([delta, delta.new_zeros(1)])          # (a pass of links without neighbours has no delta at all)
        out['deltas'].append(torch.where(have, padded[at.clamp(max=delta.numel())], padded.new_zeros(())))
        out['counts'].append(count)
    return {k: torch.cat(x, 0) for k, x in out.items()}


def explain_all(model, dataset, u, v, batch_size=50, links_per_pass=None, stats=None, capacity_variants=None,
                capacity_entries=None):
    """Every neighbour of every pair: a dict of device tensors --

    * per VARIANT (the base variants included), in the documented order: ``var_link`` int32 (index of the pair), ``var_side``
      uint8 (0 user, 1 item, 255 base), ``var_node`` int32 (-1 base), ``var_rating`` uint8, ``scores`` float32, and ``var_off``
      int64 ``[n + 1]``: pair i owns the variants ``[var_off[i], var_off[i + 1])``;
    * per ATTRIBUTION (the base variants dropped): ``delta`` float32, and ``seg_off`` int64 ``[n + 1]`` = ``var_off - arange``:
      attribution ``a`` of pair ``i`` is variant ``a + i + 1``;
    * ``base`` float32 ``[n]``."""
    keys = ('var_link', 'var_side', 'var_node', 'var_rating', 'scores', 'delta', 'base')
    out = {k: [] for k in keys}
    var_off, seg_off, nvar = [], [], 0
    for l0, L, loo, offs, scores in _variant_passes(model, dataset, u, v, batch_size, links_per_pass, capacity_variants,
                                                    capacity_entries, stats):
        base, delta, _, so = _deltas(loo, offs, scores, L)
        k = len(loo)
        for name in ('var_link', 'var_side', 'var_node', 'var_rating'):
            out[name].append(getattr(loo, name)[:k].clone())
        out['scores'].append(scores)
        out['delta'].append(delta)
        out['base'].append(base)
        var_off.append(offs[0, :-1] + nvar)
        seg_off.append(so[:-1] + (nvar - l0))
        nvar += k
    res = {k: torch.cat(x, 0) for k, x in out.items()}
    n = res['base'].numel()
    end = torch.tensor([nvar], dtype=torch.int64, device=res['base'].device)
    res['var_off'] = torch.cat(var_off + [end], 0)
    res['seg_off'] = torch.cat(seg_off + [end - n], 0)
    return res


def parse_links(lines, name='<links>'):
    """``--explain-links``: lines ``user item`` separated by whitespace, ``#`` starts a comment, blank lines are skipped (the
    format of ``new_ratings.parse_new_ratings`` without the rating).  -> ``(users int32, items int32)``; ``ValueError`` names
    the offending line.  A pure function of its arguments."""
    users, items = [], []
    for no, line in enumerate(lines, 1):
        text = line.split('#', 1)[0].strip()
        if not text:
            continue
        where = '%s, line %d' % (name, no)
        parts = text.split()
        if len(parts) != 2:
            raise ValueError('%s: expected "user item", got %r' % (where, text))
        try:
            a, b = int(parts[0]), int(parts[1])
        except ValueError:
            raise ValueError('%s: user and item are integer ids, got %r %r' % (where, parts[0], parts[1]))
        if not (0 <= a < 2 ** 31 - 1 and 0 <= b < 2 ** 31 - 1):
            raise ValueError('%s: ids must be in [0, 2^31 - 1), got %d %d' % (where, a, b))
        users.append(a)
        items.append(b)
    return np.asarray(users, np.int32), np.asarray(items, np.int32)


def read_links(path):
    with open(path) as f:
        return parse_links(f, name=path)
