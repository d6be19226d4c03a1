"""Held-out ranking evaluation on the device: where do the items a user really rated stand in that user's recommendation
list -- hit rate, recall, precision, NDCG@K and MRR over a held-out split (no reference counterpart: the reference judges
rating regression only, by the test RMSE, which says nothing about order).

Held-out links are absent from the training graph, so they are candidates of :mod:`igmc_amd.recommend` already.
:func:`rank_eval` runs the passes of ``recommend`` (``recommend.candidate_passes``: refill, score -- one ``CandidateLinks``,
one replayed ``ScoreGraph``) and, instead of taking the ``n`` best of every segment, asks where GIVEN items stand
(``igmc_amd/csrc/ranking.hip``):

* ``igmc_rank_segments`` finds every held-out item in its user's item-ascending segment by binary search and counts the
  candidates in front of it in the order of ``igmc_select_segments`` (score descending, item id ascending, NaNs last): its
  0-based rank, an integer that does not depend on the launch geometry;
* ``igmc_rank_metrics`` reduces the ranks to per-user sums (relevant links, first rank, hits@K, DCG@K, ideal DCG@K), float64
  in a fixed order.

Nothing per candidate crosses to the host: one total per pass (the refill's), the per-user query offsets of the held-out set
once, and the handful of means at the end.

THE METRICS (binary relevance; means in float64 over the users that have at least one relevant held-out link WITH A RANK):
``hr@K`` = mean(hits_K > 0), ``recall@K`` = mean(hits_K / n_rel), ``precision@K`` = mean(hits_K / K), ``ndcg@K`` =
mean(dcg_K / idcg_K), ``mrr`` = mean(1 / (first_rank + 1)), with hits_K = #{rank < K}.  ``recall@K`` IS NORMALISED BY n_rel,
NOT BY min(K, n_rel): a user with more relevant links than K cannot reach 1 (``ndcg@K``'s ideal list does stop at
min(K, n_rel)).  A held-out link that is NO CANDIDATE (the user also has it in the rating graph and ``exclude_seen`` is set,
or ``item_mask`` leaves the item out) has no rank: it is counted in ``stats['not_candidates']`` and LEFT OUT of every metric,
n_rel included -- never silently counted as a miss.  A link given twice counts twice.

SAMPLER POSITIONS.  As in :mod:`igmc_amd.recommend`: the extraction's sampler is keyed by (seed, epoch, link position), and a
candidate's position is its index in ITS PASS's list.  Where a per-hop cap binds (a neighbourhood larger than
``max_nodes_per_hop`` is sampled), a candidate's score -- and so a held-out link's RANK -- depends on where it sits in its
pass, hence on ``users_per_pass`` and on the users evaluated with it; every result is still a deterministic function of
(seed, users, ``users_per_pass``).  Where no cap binds the ranks do not depend on how the users are divided into passes.

SAMPLED NEGATIVES (``negatives=K``): the protocol most of the top-N literature reports -- every user's held-out items ranked
among K uniformly sampled unseen items (NCF's "99 negatives") instead of among all of them.  The pass's list of a user is then
its held-out items (the must items of ``recommend.CandidateLinks.refill``) and the K items of the REST of its candidates with
the smallest hash key under (the dataset's seed, ``draw``, the user id): a user's negatives do not depend on the users
evaluated with it or on ``users_per_pass``.  A user's OTHER held-out items stay in the list and compete with each of them,
exactly as they do in the exhaustive evaluation, so ``negatives`` >= every user's number of other candidates reproduces the
exhaustive result bit for bit; ranking each positive against the negatives alone is not offered.  ``not_candidates`` is what
it is in the exhaustive run.  SAMPLER POSITIONS carries over, and positions in a sampled list differ from those in the full
list: under a binding per-hop cap the sampled and the exhaustive score of the same pair may differ.

SHORTLISTS (``shortlist=M``; ``recommend``'s module docstring): only every user's M candidates with the most co-rating votes are
scored, as ``recommend(shortlist=M)`` scores them.  A held-out link that IS a candidate but is cut by the shortlist is a MISS: it
counts in n_rel, has no hit at any K, adds nothing to the DCG (the ideal DCG does count it) and its reciprocal rank is 0 -- it
carries the rank ``MISS_RANK``, beyond every K.  A link that is no candidate keeps the treatment above.  The two are told apart
by ``igmc_shortlist_places`` in the same pass (the link's place in the full vote order: ``place >= M`` is a cut), not by a second
enumeration.  M >= every user's candidate count reproduces the exhaustive result bit for bit.  :func:`shortlist_recall` judges the
shortlist by itself, without the model: the share of relevant held-out candidate links with ``place < M``.

COLD START (:func:`hold_out`, :func:`cold_start_eval`): how good is the list of a user with 1, 2, 5 or 10 ratings -- the Given-N
protocol of the collaborative-filtering literature: per user a uniform k-subset of the row is kept and everything else the user
rated is the test set.  The split runs on the device (``igmc_holdout_count`` / ``_fill``, ``igmc_amd/csrc/holdout.hip``; keyed by
(the source's seed, ``draw``, the user id), so a user's split does not depend on the users evaluated with it, and the kept
sets of the levels are NESTED: the five ratings of level 5 contain the two of level 2), the reduced graph is built on the
device (``engine.Graph.updated``) and ranked over through a ``recommend.GraphView``.  ``keep=1, hold=1`` is the NCF-style
leave-one-out split.  TWO CAVEATS about what the numbers mean:

(a) The removed links were regression targets when the model was trained.  IGMC has no per-user parameters, so what can leak
    passes through the shared weights only -- but it can.  The ``extra`` block (links of a test set the model never saw, ranked
    in the same lists) is the leak-free figure; the ``heldout`` block is not.
(b) Every evaluated user goes cold TOGETHER, and they are each other's two-hop neighbours: the reduced graph lacks the removed
    ratings of all of them.  A small ``users`` subset measures "a cold user in a warm system"; all users measures "a cold
    system".  The two differ, and neither is wrong.
"""
import numpy as np
import torch

from . import engine
from .recommend import GraphView, _check_shortlist, _dev_int32, _item_mask, candidate_passes

MISS_RANK = 2 ** 31 - 1      # the rank of a held-out candidate link that a shortlist cut: at or beyond every K (a K is below 2^31),
                             # above every real rank (a list holds fewer than 2^31 - 1 entries)


class HeldOut(object):
    """Held-out links grouped by user, on the device: ``users`` (int32 ``[nu]``, distinct, ascending), ``offsets`` (int64
    ``[nu + 1]``: user ``users[i]`` owns the links ``offsets[i]:offsets[i + 1]``), ``items`` (int32 ``[n]``, ascending
    within a user), ``relevant`` (uint8 ``[n]``, or None = every link is relevant) and ``order`` (int64 ``[n]``: the
    index in the input of the link at each place); ``source`` (uint8 ``[n]``, in the held-out order; None unless given):
    which of several link sets a link came from (``Split.heldout``: 0 = removed from the graph, 1 = of the extra set)."""

    def __init__(self, users, offsets, items, relevant, order, source=None):
        self.users, self.offsets, self.items, self.relevant, self.order = users, offsets, items, relevant, order
        self.source = source

    def __len__(self):
        return self.items.numel()

    @classmethod
    def from_links(cls, dataset_or_graph, u=None, v=None, ratings=None, min_rating=None, source=None):
        """Links ``(u[i], v[i])`` (ids, host or device) sorted by (user, item) on the device.  ``relevant = ratings >=
        min_rating``; with ``min_rating=None`` every link is relevant.  The first argument names the rating graph the ids
        belong to (a dataset or its ``engine.Graph``); a dataset given WITHOUT ``u`` / ``v`` is the held-out set itself:
        its ``link_u``, ``link_v`` and -- as ratings -- ``link_y``.  ``source``: one uint8 per link, carried along by
        ``order``."""
        src = dataset_or_graph
        graph = getattr(src, 'graph', src)
        if u is None and v is None:
            if not hasattr(src, 'link_u'):
                raise ValueError('no links: give u and v, or a dataset')
            u, v = src.link_u[:len(src)], src.link_v[:len(src)]
            if ratings is None:
                ratings = src.link_y[:len(src)]
        elif u is None or v is None:
            raise ValueError('u and v come together')
        dev = src.link_y.device if hasattr(src, 'link_y') else torch.device('cuda', graph.device)
        u, v = _dev_int32(u, dev, 'u').long(), _dev_int32(v, dev, 'v').long()
        if u.numel() != v.numel():
            raise ValueError('u and v differ in length')
        if u.numel() < 1:
            raise ValueError('no held-out links')
        if bool(((u < 0) | (u >= graph.n_users) | (v < 0) | (v >= graph.n_items)).any().item()):
            raise ValueError('a link outside the rating graph (%d users x %d items)' % (graph.n_users, graph.n_items))
        relevant = None
        if min_rating is not None:
            if ratings is None:
                raise ValueError('min_rating needs the ratings of the links')
            r = torch.as_tensor(np.asarray(ratings) if not torch.is_tensor(ratings) else ratings).to(dev)
            if r.dim() != 1 or r.numel() != u.numel():
                raise ValueError('one rating per link')
            relevant = r >= min_rating
        order = torch.argsort(u * graph.n_items + v, stable=True)
        u, v = u[order], v[order]
        users, counts = torch.unique_consecutive(u, return_counts=True)
        offsets = torch.zeros(users.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=offsets[1:])
        if source is not None:
            source = torch.as_tensor(source).to(device=dev, dtype=torch.uint8)
            if source.dim() != 1 or source.numel() != u.numel():
                raise ValueError('one source per link')
            source = source[order].contiguous()
        return cls(users.to(torch.int32), offsets, v.to(torch.int32).contiguous(),
                   None if relevant is None else relevant[order].to(torch.uint8).contiguous(), order, source)


def _select(heldout, users):
    """The held-out users to evaluate -- all of them, or those that are also in ``users`` -- as ``(users int32 [m], q_off
    int64 [m + 1], items, relevant, index)``: their links side by side, ``index`` = each link's place in ``heldout`` (None:
    all of them, as they are)."""
    if users is None:
        return heldout.users, heldout.offsets, heldout.items, heldout.relevant, None
    dev = heldout.items.device
    sel = torch.isin(heldout.users, _dev_int32(users, dev, 'users')).nonzero().view(-1)
    lens = heldout.offsets[sel + 1] - heldout.offsets[sel]
    q_off = torch.zeros(sel.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=q_off[1:])
    index = torch.repeat_interleave(heldout.offsets[sel] - q_off[:-1], lens) + \
        torch.arange(int(lens.sum().item()), dtype=torch.int64, device=dev)
    return (heldout.users[sel], q_off, heldout.items[index].contiguous(),
            None if heldout.relevant is None else heldout.relevant[index].contiguous(), index)


def metric_names(ks):
    return ['%s@%d' % (m, k) for k in ks for m in ('hr', 'recall', 'precision', 'ndcg')] + ['mrr']


def reduce_metrics(cnt, dcg, ks):
    """The means of the module docstring from the per-user sums of ``igmc_rank_metrics``: a float64 device vector in the
    order of :func:`metric_names`, with the number of users it was taken over behind it.  NaN where no user counts.  A first
    rank of ``MISS_RANK`` (every relevant link of the user was cut by a shortlist) has the reciprocal rank 0."""
    nk = len(ks)
    keep = cnt[:, 0] > 0
    n = keep.sum().to(torch.float64)
    n_rel = cnt[keep, 0].to(torch.float64)
    hits = cnt[keep, 2:].to(torch.float64)
    out = []
    for j, k in enumerate(ks):
        out += [(hits[:, j] > 0).to(torch.float64).sum() / n, (hits[:, j] / n_rel).sum() / n, (hits[:, j] / float(k)).sum() / n,
                (dcg[keep, j] / dcg[keep, nk + j]).sum() / n]
    first = cnt[keep, 1]
    rr = 1.0 / (first.to(torch.float64) + 1.0)
    out.append(torch.where(first == MISS_RANK, torch.zeros_like(rr), rr).sum() / n)
    return torch.stack(out + [n])


def rank_eval(model, dataset, heldout, ks=(5, 10, 20), batch_size=50, exclude_seen=True, item_mask=None, users=None,
              users_per_pass=None, stats=None, negatives=None, draw=0, shortlist=None, seed_min_rel=0, vote_min_rel=0):
    """Ranking metrics of ``heldout`` (a :class:`HeldOut`, or a dataset: :meth:`HeldOut.from_links`) over the rating graph
    and with the extraction settings of ``dataset`` (normally the training set), for the held-out users -- or those of
    them that are in ``users`` --: for every pass of ``recommend`` (same candidates, same scores, same ``users_per_pass``)
    the rank of every held-out link among its user's candidates, then the per-user sums and their means.

    Returns a dict of Python floats ``hr@K``, ``recall@K``, ``precision@K``, ``ndcg@K`` for every K of ``ks`` (1 to 8
    cut-offs) and ``mrr`` (see the module docstring; NaN when no user counts), ``users_evaluated`` (int: the users the means
    were taken over) and ``per_user``: device tensors ``users`` (int32 ``[m]``), ``offsets`` (int64 ``[m + 1]``: the user's
    links), ``items`` / ``relevant`` of the links, ``cnt`` (int32 ``[m, 2 + nk]``) / ``dcg`` (float64 ``[m, 2 * nk]``) as
    ``engine.rank_metrics`` returns them, and per link ``rank`` and ``pos``, its position in ITS PASS's candidate list
    (both -1 for a link that is no candidate), ``index`` (its place in ``heldout``; None = the same place).  With
    ``shortlist``: also ``place``, the link's place in its user's full vote order (-1: no candidate), and a link the shortlist
    cut has ``pos`` -1 and ``rank`` ``MISS_RANK``.

    ``negatives=K``: among ``K`` sampled negatives per user, drawn under ``draw`` (module docstring: SAMPLED NEGATIVES); the
    default ranks among every candidate.  ``shortlist=M`` (not together with ``negatives``): among the user's M candidates with
    the most co-rating votes under ``seed_min_rel`` / ``vote_min_rel``, links the shortlist cut counted as misses (module
    docstring: SHORTLISTS; a user without a seeding entry is shortlisted its M lowest candidate ids).

    ``stats`` receives ``users``, ``candidates``, ``passes``, ``queries`` and ``not_candidates`` -- and ``negatives`` and
    ``draw`` where ``negatives`` is given, ``shortlist`` and ``cut_by_shortlist`` where ``shortlist`` is.  Works for ``DGCNN_RS`` too, over a ``recommend.GraphView``, and over a dataset
    with side features (gathered per candidate from its ``node_side()`` tables)."""
    if not isinstance(heldout, HeldOut):
        heldout = HeldOut.from_links(heldout)
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= 8 or min(ks) < 1:
        raise ValueError('ks: 1 to 8 cut-offs K >= 1')
    _check_shortlist(shortlist, negatives)
    sel_users, q_off, items, relevant, index = _select(heldout, users)
    if sel_users.numel() < 1:
        raise ValueError('none of the users has a held-out link')
    dev = items.device
    bounds = q_off.tolist()                 # (per user, once: the passes' slices of the query list)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    pos, rank, place, total, passes = [], [], [], 0, 0
    sampled = {} if negatives is None else dict(negatives=int(negatives), must=(q_off, items), draw=int(draw))
    if shortlist is not None:
        sampled = dict(shortlist=int(shortlist), seed_min_rel=seed_min_rel, vote_min_rel=vote_min_rel)
        mask = _item_mask(dataset.graph, item_mask, dev)
        serr = torch.zeros(1, dtype=torch.int32, device=dev)
    for q0, cands, R in candidate_passes(model, dataset, sel_users, batch_size, exclude_seen, item_mask, users_per_pass,
                                         **sampled):
        m = cands.users.numel()
        a, b = bounds[q0], bounds[q0 + m]
        mine = (q_off[q0:q0 + m + 1] - a).contiguous()
        p, r = engine.rank_segments(R, cands.link_v[:len(cands)], cands.offsets, mine, items[a:b], err=err, lib=cands.lib)
        if shortlist is not None:          # a candidate the shortlist cut is a miss, not a link without a rank
            pl, _ = engine.shortlist_places(cands.graph, cands.users, mask, exclude_seen, mine, items[a:b].contiguous(),
                                            seed_min_rel, vote_min_rel, err=serr)
            r = torch.where((p < 0) & (pl >= 0), torch.full_like(r, MISS_RANK), r)
            place.append(pl)
        pos.append(p)
        rank.append(r)
        total += len(cands)
        passes += 1
    pos, rank = torch.cat(pos), torch.cat(rank)
    cnt, dcg = engine.rank_metrics(rank, q_off, ks, relevant, err=err, lib=dataset.graph.lib)
    means = reduce_metrics(cnt, dcg, ks)
    cut = 0
    if shortlist is not None:
        place = torch.cat(place)
        cut, bad = torch.stack([((pos < 0) & (place >= 0)).sum(), serr[0].to(torch.int64)]).tolist()
        if bad:
            raise RuntimeError('rank_eval: igmc_shortlist_places reported err=%d' % bad)
    host = torch.cat([means, (pos < 0).sum().to(torch.float64).view(1), err.to(torch.float64)]).tolist()
    if int(host[-1]):
        engine._raise_rank_errors(err, 'rank_eval')
    if stats is not None:
        stats.update(users=sel_users.numel(), candidates=total, passes=passes, queries=items.numel(),
                     not_candidates=int(host[-2]) - cut)
        if negatives is not None:
            stats.update(negatives=int(negatives), draw=int(draw))
        if shortlist is not None:
            stats.update(shortlist=int(shortlist), cut_by_shortlist=cut)
    out = dict(zip(metric_names(ks), host[:-3]))
    out['users_evaluated'] = int(host[-3])
    out['per_user'] = dict(users=sel_users, offsets=q_off, items=items, relevant=relevant, cnt=cnt, dcg=dcg, rank=rank,
                           pos=pos, index=index)
    if shortlist is not None:
        out['per_user']['place'] = place
    return out


def shortlist_recall(dataset, heldout, ms=(50, 100, 200, 500), users=None, exclude_seen=True, item_mask=None,
                     users_per_pass=65536, seed_min_rel=0, vote_min_rel=0, stats=None):
    """How much of ``heldout`` a co-rating shortlist of each size M of ``ms`` keeps -- no model, no scoring: the number a user
    needs to choose M.  Over the rating graph of ``dataset`` (a dataset or a ``recommend.GraphView``), for the held-out users
    -- or those of them in ``users`` --, ``igmc_shortlist_places`` gives every held-out link its place in its user's full
    vote order (one call per pass of ``users_per_pass`` users; the reductions run on the device, one host read at the end).
    Over the RELEVANT held-out links that are candidates (``place >= 0``; the others are left out, as ``rank_eval`` leaves
    them out), per M: ``micro`` = the share of links with ``place < M``, ``macro`` = the mean over the users that have such a
    link of the user's own share.  Returns ``{M: {'micro': x, 'macro': y}}`` (NaN where no link counts); ``stats`` receives
    ``users``, ``queries``, ``links`` (those that count), ``users_counted``, ``not_candidates`` and ``passes``.  A user
    without a seeding entry is shortlisted its M lowest candidate ids, so its links count like any other."""
    if not isinstance(heldout, HeldOut):
        heldout = HeldOut.from_links(heldout)
    ms = [int(m) for m in ms]
    if not ms or min(ms) < 1 or max(ms) > 2 ** 31 - 1:
        raise ValueError('ms: shortlist sizes in [1, 2^31)')
    sel_users, q_off, items, relevant, _ = _select(heldout, users)
    if sel_users.numel() < 1:
        raise ValueError('none of the users has a held-out link')
    dev = items.device
    g = dataset.graph
    mask = _item_mask(g, item_mask, dev)
    bounds = q_off.tolist()
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    upp = max(1, int(users_per_pass))
    place, passes = [], 0
    for q0 in range(0, sel_users.numel(), upp):
        m = min(upp, sel_users.numel() - q0)
        a, b = bounds[q0], bounds[q0 + m]
        place.append(engine.shortlist_places(g, sel_users[q0:q0 + m].contiguous(), mask, exclude_seen,
                                             (q_off[q0:q0 + m + 1] - a).contiguous(), items[a:b].contiguous(), seed_min_rel,
                                             vote_min_rel, err=err)[0])
        passes += 1
    place = torch.cat(place)
    counts = (place >= 0) if relevant is None else ((place >= 0) & (relevant != 0))
    owner = torch.repeat_interleave(torch.arange(sel_users.numel(), device=dev), q_off[1:] - q_off[:-1])
    per_user = torch.zeros(sel_users.numel(), dtype=torch.float64, device=dev).index_add_(0, owner, counts.to(torch.float64))
    have = per_user > 0
    n, nu = counts.sum().to(torch.float64), have.sum().to(torch.float64)
    out = []
    for m in ms:
        hit = (counts & (place < m)).to(torch.float64)
        mine = torch.zeros_like(per_user).index_add_(0, owner, hit)
        out += [hit.sum() / n, (mine[have] / per_user[have]).sum() / nu]
    host = torch.stack(out + [n, nu, (place < 0).sum().to(torch.float64), err[0].to(torch.float64)]).tolist()
    if int(host[-1]):
        raise RuntimeError('shortlist_recall: igmc_shortlist_places reported err=%d' % int(host[-1]))
    if stats is not None:
        stats.update(users=sel_users.numel(), queries=items.numel(), links=int(host[-4]), users_counted=int(host[-3]),
                     not_candidates=int(host[-2]), passes=passes)
    return {m: dict(micro=host[2 * i], macro=host[2 * i + 1]) for i, m in enumerate(ms)}


# ------------------------------------------------------------------ cold start: the Given-k split and the evaluation over it
def _class_values(source):
    while not hasattr(source, 'class_values') and hasattr(source, 'source'):
        source = source.source
    return getattr(source, 'class_values', None)


class Split(object):
    """A Given-k split (:func:`hold_out`), everything on the device: ``users`` (int32 ``[nq]``, as requested) and ``offsets``
    (int64 ``[nq + 1]``: user ``users[q]`` lost the links ``offsets[q]:offsets[q + 1]``); the removed links ``u`` / ``v``
    (int32), ``rel`` (uint8: the relation) and ``ratings`` (float32: ``class_values[rel]``, what ``link_y`` holds) in the
    order of the users' rows; ``graph``, the rating graph without them, and ``view``, the source's settings over it."""

    def __init__(self, dataset, users, offsets, u, v, rel, ratings, graph):
        self.users, self.offsets, self.u, self.v, self.rel, self.ratings, self.graph = users, offsets, u, v, rel, ratings, graph
        self.view = GraphView(dataset, graph)

    def __len__(self):
        return self.u.numel()

    def heldout(self, extra=None, min_rating=None):
        """The :class:`HeldOut` of the split: the removed links (``source`` 0) and -- ``extra``: a dataset, normally the test
        set -- the links of ``extra`` that belong to the split's users (``source`` 1).  ``relevant = rating >= min_rating``."""
        u, v, r = self.u, self.v, self.ratings
        source = torch.zeros(u.numel(), dtype=torch.uint8, device=u.device)
        if extra is not None:
            n = len(extra)
            eu = _dev_int32(extra.link_u[:n], u.device, 'u')
            mine = torch.isin(eu, self.users)
            u = torch.cat([u, eu[mine]])
            v = torch.cat([v, _dev_int32(extra.link_v[:n], v.device, 'v')[mine]])
            r = torch.cat([r, extra.link_y[:n].to(device=r.device, dtype=torch.float32)[mine]])
            source = torch.cat([source, torch.ones(u.numel() - source.numel(), dtype=torch.uint8, device=u.device)])
        return HeldOut.from_links(self.view, u, v, ratings=r, min_rating=min_rating, source=source)


def hold_out(dataset, users=None, keep=0, hold=None, draw=0):
    """The Given-k split of ``users`` (ids, host or device, no duplicates: ``ValueError``; default every user) over the rating
    graph of ``dataset`` (a dataset or a ``recommend.GraphView``): per user the ``keep`` entries of the row with the smallest
    hash key under (the source's ``seed``, ``draw``, the user id) stay -- the whole row where it has no more --, at most
    ``hold`` of the others (None: all of them) are removed (``include/igmc_hip.h``: ``igmc_holdout_fill`` states the
    definition).  Returns a :class:`Split`.  Two launches and ``engine.Graph.updated``; ONE host read besides that call's own:
    the total, with the duplicate flag and the count's error word beside it (the fill's word can report only what that read
    has excluded: it is sized by the total, at the prefix sums of the same counts).  No host loop over users or ratings."""
    g = dataset.graph
    dev = dataset.link_y.device
    if users is None:
        users = torch.arange(g.n_users, dtype=torch.int32, device=dev)
    else:
        users = _dev_int32(users, dev, 'users')
    nq = users.numel()
    if nq < 1:
        raise ValueError('no users')
    counts, err = engine.holdout_count(g, users, keep, hold)
    offsets = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    ordered = torch.sort(users.long()).values
    dup = (ordered[1:] == ordered[:-1]).sum()
    total, dup, e = torch.stack([offsets[-1], dup, err[0].to(torch.int64)]).tolist()
    if e:
        raise ValueError('hold_out: a user id outside the rating graph (%d users)' % g.n_users)
    if dup:
        raise ValueError('hold_out: a user is named more than once')
    if total > 2 ** 31 - 1:
        raise ValueError('hold_out: %d held-out links do not fit int32 positions' % total)
    u = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    v = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    rating = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)
    engine.holdout_fill(g, users, keep, hold, offsets, u, v, rating, err, dataset.seed, draw)
    u, v, rel = u[:total], v[:total], rating[:total] - 1
    cv = _class_values(dataset)
    if cv is None:
        ratings = rel.to(torch.float32)
    else:
        ratings = torch.as_tensor(np.asarray(cv, np.float32), device=dev)[rel.long()]
    return Split(dataset, users, offsets, u, v, rel, ratings, g.updated(u, v, torch.zeros_like(rating[:total])))


def _source_block(res, heldout, which, ks, lib):
    """The metrics of ``res`` (a :func:`rank_eval` result over ``heldout``) with only the links of source ``which`` counted as
    relevant: the same ranks, one more ``engine.rank_metrics`` + :func:`reduce_metrics`."""
    per = res['per_user']
    source = heldout.source if per['index'] is None else heldout.source[per['index']]
    rel = source == which
    if per['relevant'] is not None:
        rel &= per['relevant'] != 0
    cnt, dcg = engine.rank_metrics(per['rank'], per['offsets'], ks, rel.to(torch.uint8).contiguous(), lib=lib)
    host = reduce_metrics(cnt, dcg, ks).tolist()
    out = dict(zip(metric_names(ks), host[:-1]))
    out['users_evaluated'] = int(host[-1])
    out['per_user'] = dict(users=per['users'], offsets=per['offsets'], relevant=rel, cnt=cnt, dcg=dcg)
    return out


def cold_start_eval(model, dataset, given=(1, 2, 5, 10), users=None, extra=None, ks=(5, 10, 20), draw=0, min_rating=None,
                    stats=None, **kw):
    """Ranking metrics of users cut down to ``k`` ratings, for every level ``k`` of ``given`` (module docstring: COLD START and
    its two caveats).  EVALUATED are the requested users (default: every user; no duplicates) whose row in ``dataset.graph``
    has more than ``max(given)`` entries, so that every level holds out at least one link of the same set of users; the others
    are counted in ``stats['users_skipped']`` (``stats`` also receives ``users`` and, per level, ``removed``).

    Per level: ``hold_out(dataset, evaluated, keep=k, draw=draw)``, then :func:`rank_eval` of the split's held-out set over the
    split's view -- ``result[k]['heldout']``, a :func:`rank_eval` result.  ``extra`` (a dataset, normally the test set): its
    links of the evaluated users are ranked in the same lists (and count in the ``heldout`` block), and ``result[k]['extra']``
    holds the metrics of the SAME ranks with the extra links alone counted as relevant -- no second scoring pass;
    ``result['full']['extra']`` is plain :func:`rank_eval` of those links over the unreduced graph, the warm baseline the
    ``extra`` blocks compare with.  ``kw`` goes to :func:`rank_eval`: ``negatives``, ``shortlist``, ``seed_min_rel``,
    ``vote_min_rel``, ``batch_size``, ``users_per_pass``, ``item_mask``; the sampled negatives are drawn under ``negatives_draw``
    (default: ``draw``).  Works for ``DGCNN_RS`` and with side features as far as :func:`rank_eval` over a ``GraphView`` does."""
    bad = set(kw) - {'negatives', 'negatives_draw', 'shortlist', 'seed_min_rel', 'vote_min_rel', 'batch_size', 'users_per_pass',
                     'item_mask'}
    if bad:
        raise TypeError('cold_start_eval: unexpected arguments %s' % sorted(bad))
    kw = dict(kw)
    neg_draw = kw.pop('negatives_draw', None)
    given = [int(k) for k in given]
    if not 1 <= len(given) <= 8 or min(given) < 0 or len(set(given)) != len(given):
        raise ValueError('given: 1 to 8 distinct levels >= 0')
    g, dev = dataset.graph, dataset.link_y.device
    users = torch.arange(g.n_users, dtype=torch.int32, device=dev) if users is None else _dev_int32(users, dev, 'users')
    if users.numel() < 1:
        raise ValueError('no users')
    length, err = engine.holdout_count(g, users, 0)          # (keep 0, no limit: the rows' lengths)
    evaluated = users[length > max(given)].contiguous()
    if int(err.item()):
        raise ValueError('cold_start_eval: a user id outside the rating graph (%d users)' % g.n_users)
    if evaluated.numel() < 1:
        raise ValueError('cold_start_eval: no user has more than %d ratings' % max(given))
    if stats is not None:
        stats.update(users=evaluated.numel(), users_skipped=users.numel() - evaluated.numel(), removed={})
    kw['draw'] = int(draw if neg_draw is None else neg_draw)
    result = {}
    for k in given:
        split = hold_out(dataset, evaluated, keep=k, draw=draw)
        heldout = split.heldout(extra, min_rating)
        result[k] = dict(heldout=rank_eval(model, split.view, heldout, ks, **kw))
        if extra is not None:
            result[k]['extra'] = _source_block(result[k]['heldout'], heldout, 1, ks, g.lib)
        if stats is not None:
            stats['removed'][k] = len(split)
    if extra is not None:
        result['full'] = dict(extra=rank_eval(model, dataset, HeldOut.from_links(extra, min_rating=min_rating), ks,
                                              users=evaluated, **kw))
    return result
