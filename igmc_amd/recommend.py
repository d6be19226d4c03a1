"""Top-N unseen items per user, ranked on the device (no reference counterpart: the reference stops at the test RMSE).

Scoring a link that is absent from the rating graph is the model's normal case (test links are not in ``adj_train``), so a
recommendation is a scoring pass (:func:`igmc_amd.train_eval.score_links`) with two kernels around it
(``igmc_amd/csrc/candidates.hip``; their ctypes calls: ``engine.candidates_count`` / ``candidates_fill`` / ``select_segments``):

* ``igmc_candidates_count`` / ``igmc_candidates_fill`` write the unseen items of the requested users straight into device link
  arrays -- users in the order given, item id ascending within a user;
* ``igmc_select_segments`` takes the ``n`` best of every user's contiguous score segment in the order (score descending, item
  id ascending, NaNs last).

:class:`CandidateLinks` is the ``links.LinkSource`` in between: it shares the rating graph and the extraction settings of an
existing dataset, and its link buffers are device tensors of FIXED ADDRESS AND CAPACITY that every pass refills in place, so
the hipGraph a scoring pass captured (``stepgraph.ScoreGraph``, its buffers sized by the list's ``capacity`` whatever its
length of the moment) is replayed by every later pass.

SAMPLER POSITIONS.  The extraction's sampler is keyed by (seed, epoch, link position), and a candidate's position is its index
in ITS PASS's list.  Where a per-hop cap binds (a neighbourhood larger than ``max_nodes_per_hop`` is sampled), a candidate's
sampled subgraph -- and so its score -- depends on where it sits in its pass, hence on ``users_per_pass`` and on the users
requested with it; every result is still a deterministic function of (seed, users, ``users_per_pass``).  Where no cap binds
the extraction draws nothing and the scores do not depend on how the users are divided into passes.

SAMPLED NEGATIVES (``negatives=K``; the same kernel's sampled instantiations).  ``igmc_candidates_sample_count`` / ``_fill``
write, per user, the K unseen items with the smallest ``igmc_sample_key(igmc_negative_salt(seed, draw, user), item)`` -- a
uniform K-subset keyed by the source's ``seed``, ``draw`` and the user ID, never by the users asked for with it, by
``users_per_pass`` or by the launch -- next to the request's MUST items (``must``: the held-out items of
``rank_eval.rank_eval``), which are always listed where they are candidates and are no part of the pool the K are drawn from.
A user with fewer than K other candidates gets them all.  SAMPLER POSITIONS applies unchanged, and a candidate's position in a
sampled list is not its position in the full list: under a binding per-hop cap the sampled and the exhaustive score of the
same pair may differ.

SHORTLISTS (``shortlist=M``; ``igmc_amd/csrc/shortlist.hip``).  A retrieval stage in front of the scoring pass: per user only the
``min(M, candidates)`` candidates with the most CO-RATING VOTES are listed and scored -- votes[j] = the sum, over the other users
u', of (the items u and u' both rated at relation >= ``seed_min_rel``) x [u' rated j at relation >= ``vote_min_rel``]; order:
votes descending, item id ascending (``include/igmc_hip.h`` states the definition).  ``igmc_candidates_count`` clamped to M gives
the offsets, ``igmc_shortlist_fill`` writes the segments, item ascending like every other list.  Items nobody voted for fill a
short list by ascending id, and A USER WITHOUT A SEEDING ENTRY (no rating at all, or none at or above ``seed_min_rel``) GETS ITS M
LOWEST CANDIDATE IDS: the votes say nothing about such a user -- and neither does the model, whose subgraph for it is empty.
M >= every user's candidate count reproduces the exhaustive lists byte for byte.  SAMPLER POSITIONS applies unchanged.

``link_y`` of a candidate list is zeros: the squared-error sums a scoring pass accumulates over candidates are MEANINGLESS and
are dropped here.
"""
import numpy as np
import torch

from . import engine
from .links import LinkSource, dense_side_table, kept
from .train_eval import score_links

DEFAULT_CAPACITY = 1 << 22      # candidates of one pass where the caller names no ``users_per_pass``: 4 Mi links are 48 MB of
                                # link arrays and 48 MB of score / position buffers, and 84 000 batches of 50 per replayed pass
_INT32_MAX = 2 ** 31 - 1

_ERRORS = ((1, 'a user\'s candidates reach past the capacity of the link buffers'),
           (2, 'a user id outside [0, n_users)'),
           (4, 'segment offsets that are not the prefix sums of the counts'),
           (8, 'a must item outside [0, n_items)'),
           (16, 'must offsets that decrease or leave the must list'))


def _dev_int32(x, dev, what):
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    if t.dim() != 1:
        raise ValueError('%s: a 1-D list of ids' % what)
    if t.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8, torch.int8):
        raise ValueError('%s: integer ids, not %s' % (what, t.dtype))
    return t.to(device=dev, dtype=torch.int32).contiguous()


class GraphView(LinkSource):
    """The extraction settings of ``dataset`` over ANOTHER rating graph -- normally ``dataset.graph.updated(...)``, the
    graph after new ratings (``engine.Graph.updated``: built on the device) --, shaped like a dataset as far as
    :class:`CandidateLinks` reads one: ``graph``, ``device``, ``h``, ``sample_ratio``, ``seed``, ``max_nodes_per_hop``, a
    ``link_y`` on the dataset's device (empty: a view has no links of its own) and ``node_side()``.  :func:`recommend`,
    :func:`candidate_passes`, :func:`score_candidates` and ``rank_eval.rank_eval`` take it as they take a dataset; users and
    items the graph gained are scored from their enclosing subgraphs like any other.

    SIDE FEATURES (a dataset built with ``u_features`` / ``v_features``).  Without further arguments the view serves with the
    dataset's own per-node tables, and a user or item the graph GAINED has no row there: its features read as ZEROS.  Give
    ``u_features`` and ``v_features`` (both; scipy sparse or arrays) to name them: one row per node, at least as many rows as
    the dataset's tables and exactly their column counts (``ValueError`` otherwise); the view then builds tables of its own,
    once.  Rows beyond the arrays given read zeros as well.  Over a dataset without side features the arguments are an
    error."""

    u_features = v_features = None

    def __init__(self, dataset, graph, u_features=None, v_features=None):
        self._configure_from(dataset, graph)
        self.link_y = torch.zeros(0, dtype=torch.float32, device=dataset.link_y.device)
        if u_features is not None or v_features is not None:
            if u_features is None or v_features is None or self._side_tables is None:
                raise ValueError('u_features and v_features come together, over a dataset built with side features')
            U, V = self._side_tables
            self._take_side_tables(tuple(
                torch.from_numpy(dense_side_table(f, what, old.shape[0], old.shape[1])).to(self.link_y.device)
                for f, what, old in ((u_features, 'u_features', U), (v_features, 'v_features', V))))


class CandidateLinks(LinkSource):
    """Links without labels over the rating graph of an existing dataset (a ``links.LinkSource`` with the dataset's
    settings): ``score_links`` and ``ScoreGraph`` take it as it is.

    The link buffers hold ``capacity`` entries at fixed addresses; ``len()`` is the number of links the last
    :meth:`refill` / :meth:`set_pairs` wrote.  After :meth:`refill`, ``users`` (int32 ``[nq]``) and ``offsets`` (int64
    ``[nq + 1]``) describe the per-user segments; after :meth:`set_pairs` they are ``None``.  After a refill with
    ``negatives``, ``forced`` (uint8 ``[len()]``) is 1 where the link is a must item and 0 where it was drawn; else ``None``.
    After a refill with ``shortlist``, ``votes`` (int32 ``[len()]``: the counts are below 2^31) holds every link's co-rating
    votes; else ``None``."""
    dynamic = True          # subgraphs are extracted on the fly, under the sampling key of the pass

    def __init__(self, dataset, capacity):
        self._configure_from(dataset)
        capacity = int(capacity)
        if not 1 <= capacity <= _INT32_MAX:
            raise ValueError('capacity must be in [1, 2^31): link positions are int32')
        dev = dataset.link_y.device
        self.link_u = torch.zeros(capacity, dtype=torch.int32, device=dev)      # (zeros: user 0 / item 0, valid ids -- a replayed
        self.link_v = torch.zeros(capacity, dtype=torch.int32, device=dev)      #  launch prefetches past the end of a short pass)
        self.link_y = torch.zeros(capacity, dtype=torch.float32, device=dev)
        self.n = 0
        self.users, self.offsets, self.forced, self._forced = None, None, None, None
        self.votes, self._votes = None, None

    # ---- constructors
    @classmethod
    def for_users(cls, dataset, users, exclude_seen=True, item_mask=None, capacity=None, negatives=None, must=None, draw=0,
                  shortlist=None, seed_min_rel=0, vote_min_rel=0):
        """The candidates of ``users`` (ids, host or device; duplicates allowed, each gets its own segment): every item --
        of ``item_mask`` (bool / uint8 ``[n_items]``) where given -- that the user has no entry for in the dataset's rating
        graph (``exclude_seen``), users in the order given, item id ascending.  ``capacity``: entries of the link buffers
        (default: what these users need).  ``negatives`` / ``must`` / ``draw`` / ``shortlist`` / ``seed_min_rel`` /
        ``vote_min_rel``: see :meth:`refill`."""
        _check_shortlist(shortlist, negatives)
        dev = dataset.link_y.device
        users = _dev_int32(users, dev, 'users')
        mask = _item_mask(dataset.graph, item_mask, dev)
        if capacity is None:
            counts, _ = engine.candidates_count(dataset.graph, users, mask, exclude_seen, negatives,
                                                _must(must, users, dev, negatives))
            if shortlist is not None:
                counts = counts.clamp(max=int(shortlist))
            capacity = max(1, int(counts.sum().item()))
        self = cls(dataset, capacity)
        self.refill(users, exclude_seen, mask, negatives, must, draw, shortlist, seed_min_rel, vote_min_rel)
        return self

    @classmethod
    def from_pairs(cls, dataset, u, v, capacity=None):
        """Arbitrary (user, item) pairs, host or device: "predict these links", no labels."""
        self = cls(dataset, max(1, len(u)) if capacity is None else capacity)
        self.set_pairs(u, v)
        return self

    # ---- refilling in place
    def refill(self, users, exclude_seen=True, item_mask=None, negatives=None, must=None, draw=0, shortlist=None,
               seed_min_rel=0, vote_min_rel=0):
        """Enumerate the candidates of ``users`` into the link buffers (two launches, one host read: the total).

        ``negatives=K``: every user's ``K`` sampled candidates only (module docstring: SAMPLED NEGATIVES) under the source's
        ``seed`` and ``draw``, plus the user's must items -- ``must = (offsets int64 [nq + 1], items int32)``, device tensors:
        request ``q`` must list ``items[offsets[q]:offsets[q + 1]]`` --; ``forced`` then tells the two apart.
        ``negatives=None``: ``igmc_candidates_count`` / ``_fill``, every candidate.

        ``shortlist=M`` (not together with ``negatives``: ``ValueError``): every user's ``min(M, candidates)`` candidates with
        the most co-rating votes under the relation thresholds ``seed_min_rel`` / ``vote_min_rel`` (module docstring:
        SHORTLISTS; a user without a seeding entry gets its M lowest candidate ids); ``votes`` then holds the links' votes."""
        _check_shortlist(shortlist, negatives)
        dev = self.link_y.device
        users = _dev_int32(users, dev, 'users')
        if users.numel() < 1:
            raise ValueError('no users')
        mask = _item_mask(self.graph, item_mask, dev)
        must = _must(must, users, dev, negatives)
        counts, err = engine.candidates_count(self.graph, users, mask, exclude_seen, negatives, must)
        if shortlist is not None:
            counts = counts.clamp(max=int(shortlist))
        offsets = torch.zeros(users.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=offsets[1:])
        total = int(offsets[-1].item())
        if total > self.capacity:
            raise ValueError('%d candidates do not fit the link buffers (capacity %d)' % (total, self.capacity))
        if negatives is not None and self._forced is None:
            self._forced = torch.zeros(self.capacity, dtype=torch.uint8, device=dev)
        if shortlist is not None:
            if self._votes is None:
                self._votes = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
            engine.shortlist_fill(self.graph, users, mask, exclude_seen, int(shortlist), offsets, self.link_u, self.link_v, err,
                                  self._votes, seed_min_rel, vote_min_rel)
        else:
            engine.candidates_fill(self.graph, users, mask, exclude_seen, offsets, self.link_u, self.link_v, err, negatives,
                                   must, self.seed, draw, self._forced)
        e = int(err.item())
        if e:
            raise RuntimeError('candidate enumeration: %s (err=%d)' % ('; '.join(w for b, w in _ERRORS if e & b), e))
        self.n, self.users, self.offsets = total, users, offsets
        self.forced = None if negatives is None else self._forced[:total]
        self.votes = None if shortlist is None else self._votes[:total]
        return self

    def set_pairs(self, u, v):
        dev = self.link_y.device
        u, v = _dev_int32(u, dev, 'u'), _dev_int32(v, dev, 'v')
        if u.numel() != v.numel():
            raise ValueError('u and v differ in length')
        if u.numel() > self.capacity:
            raise ValueError('%d pairs do not fit the link buffers (capacity %d)' % (u.numel(), self.capacity))
        if u.numel():
            bad = ((u < 0) | (u >= self.graph.n_users) | (v < 0) | (v >= self.graph.n_items)).any()
            if bool(bad.item()):
                raise ValueError('a pair outside the rating graph (%d users x %d items)' % (self.graph.n_users,
                                                                                         self.graph.n_items))
        self.link_u[:u.numel()].copy_(u)
        self.link_v[:v.numel()].copy_(v)
        self.n, self.users, self.offsets, self.forced, self.votes = u.numel(), None, None, None, None
        return self

    def __len__(self):
        return self.n


def _item_mask(graph, item_mask, dev):
    if item_mask is None:
        return None
    m = torch.as_tensor(np.asarray(item_mask) if not torch.is_tensor(item_mask) else item_mask)
    if m.dim() != 1 or m.numel() != graph.n_items:
        raise ValueError('item_mask: one entry per item (%d)' % graph.n_items)
    return (m != 0).to(device=dev, dtype=torch.uint8).contiguous()


def _check_shortlist(shortlist, negatives):
    if shortlist is None:
        return
    if negatives is not None:
        raise ValueError('shortlist and negatives exclude one another: a sampled list is an evaluation protocol, a shortlist '
                         'a retrieval stage')
    if not 1 <= int(shortlist) <= _INT32_MAX:
        raise ValueError('shortlist must be in [1, 2^31)')


def _must(must, users, dev, negatives):
    """``must`` of :meth:`CandidateLinks.refill` as contiguous device tensors ``(offsets int64 [nq + 1], items int32)``, or
    None."""
    if must is None:
        return None
    if negatives is None:
        raise ValueError('must items come with negatives=K: an exhaustive list holds every candidate already')
    off, items = must
    off = torch.as_tensor(off).to(device=dev, dtype=torch.int64).contiguous()
    items = torch.as_tensor(items).to(device=dev, dtype=torch.int32).contiguous()
    if off.dim() != 1 or off.numel() != users.numel() + 1 or items.dim() != 1:
        raise ValueError('must: (offsets [nq + 1], items), one offset range per requested user')
    return off, items


def score_candidates(model, cands, batch_size=50):
    """One prediction per candidate of ``cands``: a float32 device tensor of ``len(cands)`` entries in the list's order,
    computed by ``score_links`` under the sampling key ``SCORE_EPOCH`` (position = index in the list)."""
    B = int(batch_size)
    if len(cands) < 1:
        return torch.zeros(0, dtype=torch.float32, device=cands.link_y.device)
    R, _, _ = score_links(model, cands, B)          # (labels are zeros: the squared-error sums mean nothing)
    return R


def top_n(cands, scores, n, geometry=0):
    """The ``n`` best candidates of every user of ``cands`` (after ``for_users`` / ``refill``) by ``scores`` (what
    :func:`score_candidates` returned): ``(items int32 [nq, n], scores float32 [nq, n], counts int32 [nq])`` on the device.
    Order: score descending, then item id ascending, NaNs last; a user with fewer than ``n`` candidates has ``count < n``,
    items padded with -1 and scores with 0.  ``igmc_select_segments`` + one gather of ``link_v``."""
    if cands.offsets is None:
        raise ValueError('top_n needs per-user segments: a CandidateLinks filled by for_users() / refill()')
    n = int(n)
    if not 1 <= n <= 64:
        raise ValueError('n must be in [1, 64]')
    if scores.numel() != len(cands):
        raise ValueError('one score per candidate: %d scores, %d candidates' % (scores.numel(), len(cands)))
    idx, key, count = engine.select_segments(scores, cands.offsets, n, geometry, lib=cands.lib)
    have = idx >= 0
    items = torch.where(have, cands.link_v[:max(len(cands), 1)][idx.clamp(min=0).long()], torch.full_like(idx, -1))
    return items, key, count


def pass_plan(graph, n_users_requested, item_mask=None, users_per_pass=None, per_user=None):
    """``(users_per_pass, capacity)`` of :func:`recommend`: by default the largest number of users whose WORST-CASE candidate
    count (every item, or every item of the mask; with sampled negatives at most ``per_user`` = negatives + the longest must
    list, with a shortlist ``per_user`` = its size) stays within ``DEFAULT_CAPACITY`` -- at least one user, at most those requested --; positions stay below 2^31 in
    every case."""
    worst = max(1, graph.n_items if item_mask is None else int((torch.as_tensor(item_mask) != 0).sum().item()))
    if per_user is not None:
        worst = max(1, min(worst, int(per_user)))
    if users_per_pass is None:
        upp = max(1, min(int(n_users_requested), DEFAULT_CAPACITY // worst))
    else:
        upp = max(1, min(int(users_per_pass), int(n_users_requested)))
    if upp * worst > _INT32_MAX:
        raise ValueError('%d users x %d items per pass: link positions must stay below 2^31' % (upp, worst))
    return upp, upp * worst


def candidate_passes(model, dataset, users=None, batch_size=50, exclude_seen=True, item_mask=None, users_per_pass=None,
                     negatives=None, must=None, draw=0, shortlist=None, seed_min_rel=0, vote_min_rel=0):
    """The pass loop of :func:`recommend` and of ``rank_eval.rank_eval``: ``users`` (default: every user of the rating graph)
    in passes of ``users_per_pass`` (:func:`pass_plan`); a generator of ``(q0, cands, scores)`` -- the index of the pass's
    first user in ``users``, the ONE :class:`CandidateLinks` every pass refills (kept as ``dataset._recommend_links`` and
    reused by later calls that fit it, so every pass replays one captured ``ScoreGraph``) and the pass's scores
    (:func:`score_candidates`).  ``cands`` is refilled by the next pass: take what you need from it before asking for it.
    ``negatives`` / ``must`` / ``draw``: sampled lists (:meth:`CandidateLinks.refill`); ``must`` covers all of ``users`` and
    every pass gets its slice (one host read of the offsets), and the passes are planned for ``negatives`` + the longest must
    list per user instead of every item.  ``shortlist`` / ``seed_min_rel`` / ``vote_min_rel``: co-rating shortlists
    (module docstring: SHORTLISTS); the passes are planned for ``min(shortlist, items)`` per user."""
    from . import train_eval
    _check_shortlist(shortlist, negatives)
    if model.flat_parameters().device.type != train_eval.device.type:
        model.to(train_eval.device)
    dev = dataset.link_y.device
    g = dataset.graph
    users = torch.arange(g.n_users, dtype=torch.int32, device=dev) if users is None else _dev_int32(users, dev, 'users')
    nq = users.numel()
    if nq < 1:
        raise ValueError('no users')
    mask = _item_mask(g, item_mask, dev)
    must = _must(must, users, dev, negatives)
    per_user, bounds = None, None
    if negatives is not None:
        bounds = None if must is None else must[0].tolist()
        per_user = int(negatives) + (max(b - a for a, b in zip(bounds[:-1], bounds[1:])) if bounds else 0)
    if shortlist is not None:
        per_user = int(shortlist)
    upp, capacity = pass_plan(g, nq, mask, users_per_pass, per_user)
    cands = kept(dataset, '_recommend_links', lambda c: c.capacity >= capacity, lambda: CandidateLinks(dataset, capacity))
    for q0 in range(0, nq, upp):
        mine = None
        if bounds is not None:
            m = min(upp, nq - q0)
            mine = ((must[0][q0:q0 + m + 1] - bounds[q0]).contiguous(), must[1][bounds[q0]:bounds[q0 + m]])
        cands.refill(users[q0:q0 + upp], exclude_seen, mask, negatives, mine, draw, shortlist, seed_min_rel, vote_min_rel)
        yield q0, cands, score_candidates(model, cands, batch_size)


def recommend(model, dataset, users=None, n=10, batch_size=50, exclude_seen=True, item_mask=None, users_per_pass=None,
              stats=None, shortlist=None, seed_min_rel=0, vote_min_rel=0):
    """Ranked top-``n`` items for ``users`` (default: every user of the rating graph) over the rating graph and with the
    extraction settings of ``dataset`` (normally the training set): ``(items int32 [nq, n], scores float32 [nq, n], counts
    int32 [nq])``, device tensors, rows in the order of ``users``, -1 / 0 behind a user's count.

    ``exclude_seen``: items the user has an entry for in the rating graph are no candidates.  ``item_mask``: bool / uint8
    ``[n_items]``, candidates are drawn from its items only.  The work is done in passes of ``users_per_pass`` users
    (:func:`pass_plan`); all passes refill ONE :class:`CandidateLinks` -- kept as ``dataset._recommend_links`` and reused by
    later calls that fit it -- and therefore replay one captured ``ScoreGraph`` (:func:`candidate_passes`).  Nothing per
    candidate crosses to the host: one total per pass does.  Works for ``DGCNN_RS`` too (``score_links``' eager path).

    Where a per-hop cap binds, scores depend on ``users_per_pass`` (see the module docstring: SAMPLER POSITIONS).
    ``shortlist=M``: only every user's M candidates with the most co-rating votes are scored (module docstring: SHORTLISTS; a
    user without a seeding entry gets its M lowest candidate ids); M >= every candidate count is the exhaustive result.
    ``stats``: a dict that receives ``users``, ``candidates`` and ``passes`` -- and ``shortlist`` where one is given."""
    items, scores, counts, total, nq = [], [], [], 0, 0
    for _, cands, R in candidate_passes(model, dataset, users, batch_size, exclude_seen, item_mask, users_per_pass,
                                        shortlist=shortlist, seed_min_rel=seed_min_rel, vote_min_rel=vote_min_rel):
        total += len(cands)
        nq += cands.users.numel()
        i, s, c = top_n(cands, R, n)
        items.append(i)
        scores.append(s)
        counts.append(c)
    if stats is not None:
        stats.update(users=nq, candidates=total, passes=len(items))
        if shortlist is not None:
            stats.update(shortlist=int(shortlist))
    return torch.cat(items, 0), torch.cat(scores, 0), torch.cat(counts, 0)
