"""Pair training: fine-tune a rating regressor for RANKING (no reference counterpart: the reference trains on observed links
with MSE and never sees an unobserved (user, item) pair).

Every training link (u, i) is paired, anew every epoch, with an item j the user has not rated, drawn on the device
(``igmc_pair_negatives``), and the step's objective is that the observed link scores higher:

    softplus(-(s(u, i) - s(u, j)))  +  mse_weight * (s(u, i) - rating)^2,   mean over the valid pairs,  + ARR

``mse_weight = 1`` (the default) keeps the tuned model's scores ratings -- ``recommendations_*.tsv`` prints them and ``--explain``
reports deltas in rating units --, ``mse_weight = 0`` is the plain BPR objective.  A step is eager: extraction, edge dropout,
``igmc_pair_loss_grad`` (training forward, pair loss, backward of the generic sequence), ``FlatAdam.step``; nothing is read back
inside an epoch.  The fused step of ``train_eval.train`` is not involved: its loss head forms ``out - y`` inside the launch that
runs the backward, and a pair's gradient needs the partner's score first.

* :class:`PairLinks`   the link list of (positive, negative) slots over a dataset's rating graph
* :func:`train_pairs`  the loop
* :func:`eval_pairs`   mean pair term / pair accuracy of a drawn list in evaluation mode
* :func:`eval_pairs_by_kind`  the same per kind of negative: uniform draws and shortlist items

HARD NEGATIVES (``train_pairs(shortlist=M, hard_share=P)``).  Behind ``--shortlist`` the ranker only ever orders the M unseen
items the co-rating votes put in front of it; a uniform draw over the catalogue almost never lands on one of them.  With a
table of every user's shortlist (:meth:`PairLinks.set_shortlist`, built once through ``recommend.CandidateLinks``) the share P
of an epoch's pairs takes its negative from the user's own list instead -- ``igmc_pair_negatives_shortlist``, label 2 --, the
rest stays uniform, and so does every pair whose pick does not qualify.
"""
import time

import numpy as np
import torch

from . import engine, parallel
from .links import LinkSource

_INT32_MAX = 2 ** 31 - 1
_M64 = (1 << 64) - 1


class PairLinks(LinkSource):
    """``2 n`` link positions over the rating graph of ``dataset``: position ``2 k`` is positive ``k`` with its rating as the
    label, position ``2 k + 1`` its negative of the current draw (:meth:`redraw`) with the label 1, or 0 where the pair is
    void -- the user has no unseen item; the slot then repeats the positive so that it stays extractable.

    The positives are the dataset's own links, or ``(u, v, y)`` (host or device arrays: user ids, item ids, rating values).
    Storage is allocated once.  Subgraphs are always extracted from the graph, under the sampling key of the epoch where the
    dataset is dynamic -- a negative has no cached node sets --, and side features are gathered by node id from the
    dataset's ``node_side()`` tables."""

    def __init__(self, dataset, u=None, v=None, y=None):
        self._configure_from(dataset)
        self.dynamic = bool(getattr(dataset, 'dynamic', True))
        dev = dataset.link_y.device
        if u is None:
            u, v, y = dataset.link_u[:len(dataset)], dataset.link_v[:len(dataset)], dataset.link_y[:len(dataset)]
        to = lambda x, dt: torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(device=dev, dtype=dt).contiguous()
        self.pos_u, self.pos_v, y = to(u, torch.int32), to(v, torch.int32), to(y, torch.float32)
        n = self.pos_u.numel()
        if not (self.pos_v.numel() == n and y.numel() == n and self.pos_u.dim() == 1):
            raise ValueError('u, v and y: 1-D arrays of one length')
        if not 1 <= n <= _INT32_MAX // 2:
            raise ValueError('between 1 and 2^30 - 1 positives: the 2 n link positions are int32')
        bad = (self.pos_u < 0) | (self.pos_u >= self.graph.n_users) | (self.pos_v < 0) | (self.pos_v >= self.graph.n_items)
        if bool(bad.any().item()):
            raise ValueError('a positive outside the rating graph (%d users x %d items)' % (self.graph.n_users,
                                                                                            self.graph.n_items))
        self.n_pairs = n
        self.link_u = self.pos_u.repeat_interleave(2).contiguous()      # (valid links before the first draw: every pair void)
        self.link_v = self.pos_v.repeat_interleave(2).contiguous()
        self.link_y = torch.zeros(2 * n, dtype=torch.float32, device=dev)
        self.link_y[0::2] = y
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.epoch = None
        self.sl_off = self.sl_item = self.shortlist = None

    def _item_mask(self, item_mask):
        if item_mask is None:
            return None
        mask = torch.as_tensor(np.asarray(item_mask) if not torch.is_tensor(item_mask) else item_mask)
        if mask.dim() != 1 or mask.numel() != self.graph.n_items:
            raise ValueError('item_mask: one entry per item (%d)' % self.graph.n_items)
        return (mask != 0).to(device=self.link_y.device, dtype=torch.uint8).contiguous()

    def set_shortlist(self, m, seed_min_rel=0, vote_min_rel=0, item_mask=None):
        """Build the table hard negatives are drawn from, ONCE: every user's co-rating shortlist of ``m`` unseen items over the
        dataset's rating graph (``recommend.CandidateLinks.refill(users = 0 .. n_users - 1, shortlist = m)``: ``exclude_seen``,
        the thresholds ``seed_min_rel`` / ``vote_min_rel``, ``item_mask``), in passes where one list of links would not hold
        them.  Offsets (int64 ``[n_users + 1]``, by user id) and items (int32) stay on the device; the only host reads are the
        passes' totals.  The table belongs to this graph and this mask: a redraw under another mask reports picks the mask
        drops as stale (``err`` bit 2) and falls back to the uniform draw."""
        from .recommend import CandidateLinks, pass_plan
        m = int(m)
        if not 1 <= m <= _INT32_MAX:
            raise ValueError('shortlist size must be in [1, 2^31)')
        dev = self.link_y.device
        mask = self._item_mask(item_mask)
        nu = self.graph.n_users
        users = torch.arange(nu, dtype=torch.int32, device=dev)
        upp, capacity = pass_plan(self.graph, nu, mask, None, m)
        cands = CandidateLinks(self.source, capacity)
        offs, items, base = [torch.zeros(1, dtype=torch.int64, device=dev)], [], 0
        for q0 in range(0, nu, upp):
            cands.refill(users[q0:q0 + upp], True, mask, shortlist=m, seed_min_rel=seed_min_rel, vote_min_rel=vote_min_rel)
            offs.append(cands.offsets[1:] + base)
            items.append(cands.link_v[:len(cands)].clone())
            base += len(cands)
        if base > _INT32_MAX:
            raise ValueError('%d shortlist entries: the table holds fewer than 2^31' % base)
        self.sl_off = torch.cat(offs).contiguous()
        self.sl_item = torch.cat(items).contiguous() if base else torch.zeros(1, dtype=torch.int32, device=dev)
        self.sl_total, self.shortlist = base, m
        return self

    def clear_shortlist(self):
        """Drop the table of :meth:`set_shortlist`: every later draw is uniform."""
        self.sl_off = self.sl_item = self.shortlist = None
        return self

    def redraw(self, epoch, item_mask=None, stream=None, hard_share=None):
        """The negatives of ``epoch`` into the odd positions (one launch, nothing read back): a function of (seed, epoch,
        position of the positive) -- the same epoch twice gives the same bytes.  ``item_mask`` (bool / uint8 ``[n_items]``):
        the items a negative may be.  ``err`` collects bit 1 where a pair is void.

        ``hard_share`` in (0, 1], after :meth:`set_shortlist`: that share of the pairs asks the user's shortlist for ONE item
        first (``igmc_pair_negatives_shortlist``; ``include/igmc_hip.h`` states the definition) and falls back to the uniform
        draw where it does not qualify.  The odd label slots then hold 1 (a uniform negative), 2 (one from the shortlist) or
        0 (void); ``err`` gains bit 2 (a stale table) and bit 3 (broken offsets).  Without a table, or with ``hard_share`` None
        or 0, this is ``igmc_pair_negatives`` and its bytes."""
        mask = self._item_mask(item_mask)
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        share = 0.0 if hard_share is None else float(hard_share)
        if not 0.0 <= share <= 1.0:
            raise ValueError('hard_share must be in [0, 1]')
        if self.sl_off is None or share == 0.0:
            engine.pair_negatives(self.graph, self.pos_u.data_ptr(), self.pos_v.data_ptr(), self.n_pairs,
                                  None if mask is None else mask.data_ptr(), self.seed, int(epoch), self.link_u.data_ptr(),
                                  self.link_v.data_ptr(), self.link_y.data_ptr(), self.err.data_ptr(), st)
        else:
            engine.pair_negatives_shortlist(self.graph, self.pos_u.data_ptr(), self.pos_v.data_ptr(), self.n_pairs,
                                            None if mask is None else mask.data_ptr(), self.seed, int(epoch),
                                            self.sl_off.data_ptr(), self.sl_item.data_ptr(), self.sl_total, share,
                                            self.link_u.data_ptr(), self.link_v.data_ptr(), self.link_y.data_ptr(),
                                            self.err.data_ptr(), st)
        self._mask = mask          # (kept until the next draw: the launch reads it)
        self.epoch = int(epoch)
        return self

    def epoch_positions(self, epoch):
        """A permutation of the PAIRS under (seed, epoch), expanded to ``[2 p, 2 p + 1]``: device int32 ``[2 n]``; the two slots
        of a pair stay adjacent, so every even-sized batch cut at an even offset holds whole pairs."""
        gen = torch.Generator()
        gen.manual_seed((self.seed * 0x9E3779B97F4A7C15 + int(epoch) * 7919 + 0x50414952) & (_M64 >> 1))
        p = torch.randperm(self.n_pairs, generator=gen)
        pos = torch.stack([2 * p, 2 * p + 1], 1).reshape(-1)
        return pos.to(device=self.link_y.device, dtype=torch.int32)


def _as_pairs(dataset):
    return dataset if isinstance(dataset, PairLinks) else PairLinks(dataset)


def _refuse(model):
    from .models import DGCNN_RS, IGMC
    if parallel.world_size() > 1:
        raise RuntimeError('pair training runs on one rank: data-parallel pair steps are not built (world size %d)'
                           % parallel.world_size())
    if isinstance(model, DGCNN_RS) or not isinstance(model, IGMC):
        raise NotImplementedError('pair training is built for IGMC (centre-node readout), not for %s' % type(model).__name__)


def train_pairs(model, dataset, epochs, batch_size, lr, mse_weight=1.0, ARR=0.001, logger=None, shortlist=None, hard_share=0.5,
                seed_min_rel=0, vote_min_rel=0):
    """Fine-tune ``model`` for ``epochs`` epochs on the pairs of ``dataset`` (a dataset: its own links are the positives; or a
    :class:`PairLinks`).  ``batch_size`` counts subgraphs and is rounded down to even.  Per epoch: one draw of the negatives,
    then eager steps with no host synchronisation; the statistics accumulate on the device and are read once.  Prints and
    returns per epoch ``dict(epoch, pair_loss, mse, pair_acc, pairs, void, steps, seconds)``: the mean pair term, the positives'
    mean squared error and ordered / valid pairs -- all over the epoch's valid pairs, under dropout, as the steps saw them --,
    and the epoch's steps and wall-clock time.
    ``logger(info)`` is called with each.

    ``shortlist=M``: HARD negatives.  Every user's co-rating shortlist of M unseen items (:meth:`PairLinks.set_shortlist` under
    ``seed_min_rel`` / ``vote_min_rel``) is built before epoch 1 and never again, and every epoch's draw asks it for the share
    ``hard_share`` of the pairs (:meth:`PairLinks.redraw`) -- 0.5 is a first value, not a tuned one.  ``igmc_pair_kind_stats``
    runs behind every step and accumulates on the device; the epoch's dict gains ``hard_pairs`` (valid pairs whose negative
    came from the shortlist), ``pair_acc_hard`` / ``pair_acc_uniform`` (ordered / valid, per kind) and ``stale`` (the sampler
    met a table that does not belong to the graph: raised here, since this function built it).  Without ``shortlist`` nothing
    of this happens: the dict, the printed line and the launches of a step are as they were."""
    from .train_eval import FlatAdam, _check_workspaces
    _refuse(model)
    B = int(batch_size) // 2 * 2
    if B < 2:
        raise ValueError('batch_size must be at least 2: a step holds whole pairs')
    if int(epochs) < 1:
        raise ValueError('epochs must be at least 1')
    pairs = _as_pairs(dataset)
    dev = pairs.link_y.device
    model.to(dev).train()
    opt = FlatAdam(model, lr=lr)
    step_stats = torch.zeros(5, dtype=torch.float64, device=dev)
    total = torch.zeros(5, dtype=torch.float64, device=dev)
    out, gout = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
    n = 2 * pairs.n_pairs
    history = []
    hard = shortlist is not None
    if hard:
        if not 0.0 <= float(hard_share) <= 1.0:
            raise ValueError('hard_share must be in [0, 1]')
        pairs.set_shortlist(shortlist, seed_min_rel, vote_min_rel)          # once: the graph does not change under the epochs
        # the loss statistics and the kinds' in ONE device array: still one read an epoch
        total = torch.zeros(11, dtype=torch.float64, device=dev)
        kind_stats = torch.zeros(6, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for epoch in range(1, int(epochs) + 1):
        t0 = time.perf_counter()
        pairs.err.zero_()
        pairs.redraw(epoch, hard_share=hard_share if hard else None)
        perm = pairs.epoch_positions(epoch)
        total.zero_()
        for first in range(0, n, B):
            data = pairs.extract(perm, first, min(B, n - first), epoch=epoch, max_graphs=B)
            model.pair_loss_grad(data, ARR=ARR, mse_weight=mse_weight, stats=step_stats, out=out, gout=gout)
            if hard:
                engine.pair_kind_stats(pairs.lib, out.data_ptr(), data.arena.device_ptr('Y'), data.num_graphs,
                                       kind_stats.data_ptr(), stream)          # (the arena's labels: what the loss read)
                total[:5] += step_stats
                total[5:] += kind_stats
            else:
                total += step_stats
            opt.step()
        t, err = total.cpu().numpy(), int(pairs.err.item())      # (the epoch's one read)
        _check_workspaces(model)
        ok = max(t[3], 1.0)
        info = dict(epoch=epoch, pair_loss=float(t[0] / ok), mse=float(t[1] / ok), pair_acc=float(t[2] / ok), pairs=int(t[3]),
                    void=pairs.n_pairs - int(t[3]), steps=(n + B - 1) // B, seconds=time.perf_counter() - t0)
        if err & 1:
            raise RuntimeError('pair sampler: a positive outside the rating graph (err=%d)' % err)
        if hard:
            info.update(hard_pairs=int(t[8]), pair_acc_hard=float(t[9] / max(t[8], 1.0)),
                        pair_acc_uniform=float(t[6] / max(t[5], 1.0)), stale=bool(err & 12))
            if info['stale']:
                raise RuntimeError('pair sampler: the shortlist table does not belong to the rating graph (err=%d)' % err)
            print('Pair epoch {}, pair loss {:.6f}, mse {:.6f}, pair acc {:.6f}, hard {:.6f}, pair acc hard {:.6f}, uniform {:.6f}'
                  .format(epoch, info['pair_loss'], info['mse'], info['pair_acc'], info['hard_pairs'] / max(info['pairs'], 1),
                          info['pair_acc_hard'], info['pair_acc_uniform']))
        else:
            print('Pair epoch {}, pair loss {:.6f}, mse {:.6f}, pair acc {:.6f}'.format(epoch, info['pair_loss'], info['mse'],
                                                                                        info['pair_acc']))
        history.append(info)
        if logger is not None:
            logger(info)
    steps, seconds = sum(h['steps'] for h in history), sum(h['seconds'] for h in history)
    print('Pair training: {} steps of {} subgraphs in {:.3f} s, {:.1f} steps/s'.format(steps, B, seconds, steps / max(seconds, 1e-9)))
    return history


def _pair_differences(model, pairs, batch_size):
    """float64 ``[n_pairs]``: s(positive) - s(negative) of the list as drawn, in evaluation mode, in the list's own order."""
    _refuse(model)
    B = int(batch_size) // 2 * 2
    was_training = model.training
    model.eval()
    n = 2 * pairs.n_pairs
    scores = torch.empty(n, dtype=torch.float32, device=pairs.link_y.device)
    with torch.no_grad():
        for first in range(0, n, B):
            data = pairs.extract(None, first, min(B, n - first), epoch=pairs.epoch or 0, max_graphs=B)
            scores[first:first + data.num_graphs] = model(data)
    model.train(was_training)
    s = scores.double()
    return s[0::2] - s[1::2]


def _term_and_accuracy(d, ok):
    k = max(int(ok.sum().item()), 1)
    term = torch.nn.functional.softplus(-d)[ok].sum().item() / k
    return term, float((d[ok] > 0).sum().item()) / k


def eval_pairs(model, pairs, batch_size=50):
    """``(mean pair term, pair accuracy)`` of the list as drawn (:meth:`PairLinks.redraw`), scored in evaluation mode -- no
    dropout -- in the list's own order; over the valid pairs.  The scores come from the model's forward; the two means over a
    list's worth of numbers are formed in float64."""
    return _term_and_accuracy(_pair_differences(model, pairs, batch_size), pairs.link_y[1::2] != 0)


def eval_pairs_by_kind(model, pairs, batch_size=50):
    """:func:`eval_pairs` per kind of negative: ``{1: (mean pair term, pair accuracy, count), 2: (...)}`` over the pairs whose
    negative is a uniform draw (label 1) and over those whose negative came from the shortlist (label 2); a kind without a
    pair gives ``(0.0, 0.0, 0)``."""
    d = _pair_differences(model, pairs, batch_size)
    by = {}
    for kind in (1, 2):
        ok = pairs.link_y[1::2] == float(kind)
        by[kind] = _term_and_accuracy(d, ok) + (int(ok.sum().item()),)
    return by
