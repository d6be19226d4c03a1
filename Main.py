"""IGMC experiment driver on the MI355X engine -- same command line, result files and log format as the
reference's ``Main.py`` (flags: reference ``Main.py:49-136``; outputs ``results/<name><appendix>_<mode>/
{log.txt,cmd_input.txt,model_checkpointN.pth,optimizer_checkpointN.pth}``: ``Main.py:31-45,188-210``).

    python Main.py --data-name ml_1m --save-appendix _mnph100 --data-appendix _mnph100 --max-nodes-per-hop 100 \
        --testing --epochs 40 --save-interval 5 --adj-dropout 0 --lr-decay-step-size 20 --ensemble --dynamic-train

Multi-GPU (one process per GPU, RCCL gradient all-reduce):
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 Main.py ...

Differences from the reference script, on purpose: the crash paths it has as shipped (``rmse`` undefined
without ``--ensemble``, ``args.epoch``: ``Main.py:471-472``) are fixed -- the value returned by
``train_multiple_epochs`` is used; ``--visualize`` (reference ``Main.py:423-435``) scores the test links on the GPU and
keeps the scores there, selects the extremes on the device and draws the subgraphs it scored; MovieLens is read from ``raw_data/`` when an
operator provides it and otherwise replaced by the MovieLens-shaped synthetic generator (no network here).
"""
from __future__ import print_function

import argparse
import math
import os
import random
import sys
from shutil import rmtree

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from igmc_amd.hostcpu import limit_host_threads  # noqa: E402

limit_host_threads()          # before numpy / torch: pools sized for the container's CPU quota, not the visible CPUs

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(int(os.environ['OMP_NUM_THREADS']))

from igmc_amd import parallel  # noqa: E402
from igmc_amd.models import IGMC
from igmc_amd.preprocessing import create_trainvaltest_split, load_data_monti, load_official_trainvaltest_split
from igmc_amd.train_eval import test_once, train_multiple_epochs, visualize
from igmc_amd.util_functions import MyDataset, MyDynamicDataset


def build_parser():
    p = argparse.ArgumentParser(description='Inductive Graph-based Matrix Completion (MI355X engine)')
    # general settings
    p.add_argument('--testing', action='store_true', default=False,
                   help='if set, use testing mode which splits all ratings into train/test; otherwise train/val/test')
    p.add_argument('--no-train', action='store_true', default=False, help='skip training, only test')
    p.add_argument('--debug', action='store_true', default=False, help='use 1000 links per split')
    p.add_argument('--data-name', default='ml_100k', help='dataset name')
    p.add_argument('--data-appendix', default='', help='appendix of the data cache directory name')
    p.add_argument('--save-appendix', default='', help='appendix of the results directory name')
    p.add_argument('--max-train-num', type=int, default=None)
    p.add_argument('--max-val-num', type=int, default=None)
    p.add_argument('--max-test-num', type=int, default=None)
    p.add_argument('--seed', type=int, default=1, metavar='S')
    p.add_argument('--data-seed', type=int, default=1234, metavar='S')
    p.add_argument('--reprocess', action='store_true', default=False)
    p.add_argument('--dynamic-train', action='store_true', default=False,
                   help='re-sample enclosing subgraphs every epoch (MyDynamicDataset)')
    p.add_argument('--dynamic-test', action='store_true', default=False)
    p.add_argument('--dynamic-val', action='store_true', default=False)
    p.add_argument('--keep-old', action='store_true', default=False)
    p.add_argument('--save-interval', type=int, default=10)
    # subgraph extraction settings
    p.add_argument('--hop', default=1, metavar='S')
    p.add_argument('--sample-ratio', type=float, default=1.0)
    p.add_argument('--max-nodes-per-hop', default=10000)
    p.add_argument('--use-features', action='store_true', default=False,
                   help='side features of the two target nodes in the MLP head (reference Main.py:94); --recommend, '
                        '--rank-eval and --explain gather them on the device by node id')
    # edge dropout settings
    p.add_argument('--adj-dropout', type=float, default=0.2)
    p.add_argument('--force-undirected', action='store_true', default=False)
    # optimization settings
    p.add_argument('--continue-from', type=int, default=None)
    p.add_argument('--lr', type=float, default=1e-3, metavar='LR')
    p.add_argument('--lr-decay-step-size', type=int, default=50)
    p.add_argument('--lr-decay-factor', type=float, default=0.1)
    p.add_argument('--epochs', type=int, default=80, metavar='N')
    p.add_argument('--batch-size', type=int, default=50, metavar='N')
    p.add_argument('--test-freq', type=int, default=1, metavar='N')
    p.add_argument('--ARR', type=float, default=0.001)
    # transfer learning, ensemble, visualization
    p.add_argument('--dgcnn-rs', action='store_true', default=False,
                   help='train DGCNN_RS (sort-pool readout, reference models.py:123-167) instead of IGMC')
    p.add_argument('--k', type=float, default=0.6,
                   help='sort-pool size of DGCNN_RS: a percentile of the subgraph sizes if < 1 (reference Main.py:369)')
    p.add_argument('--transfer', default='')
    p.add_argument('--num-relations', type=int, default=5)
    p.add_argument('--multiply-by', type=int, default=1)
    p.add_argument('--visualize', action='store_true', default=False)
    p.add_argument('--recommend', type=int, default=0, metavar='N',
                   help='write the N best unseen items of every requested user (ranked on the device) and stop; 0 = off')
    p.add_argument('--recommend-users', default=None, metavar='K|FILE',
                   help='users to recommend for: the first K user ids, or a text file with one id per line (default: all)')
    p.add_argument('--rank-eval', default=None, metavar='K[,K...]',
                   help='rank the held-out links (test split under --testing, else validation split) among every user\'s '
                        'unseen items on the device, write hr / recall / precision / ndcg @K and mrr, and stop; uses '
                        '--recommend-users to restrict the users')
    p.add_argument('--rank-negatives', type=int, default=None, metavar='K',
                   help='--rank-eval: rank every held-out link among K uniformly sampled unseen items of its user (drawn on '
                        'the device; the user\'s other held-out items stay in the list) instead of among all of them')
    p.add_argument('--rank-draw', type=int, default=0, metavar='D',
                   help='--rank-negatives: which draw of the negatives (default 0); another D gives another sample')
    p.add_argument('--cold-start', default=None, metavar='K[,K...]',
                   help='--rank-eval: the Given-K cold-start evaluation instead -- per level K every chosen user is cut down to '
                        'K ratings ON THE DEVICE (a uniform K-subset of the row stays), the removed ratings and the held-out '
                        'links are ranked over the reduced graph; writes coldstart_<data>.tsv; users with no more than max(K) '
                        'ratings are skipped.  1 to 8 levels >= 0.  Not with --new-ratings')
    p.add_argument('--cold-users', default=None, metavar='K|FILE',
                   help='--cold-start: the users that go cold, as --recommend-users names users (default: all -- "a cold '
                        'system"; a few -- "a cold user in a warm system")')
    p.add_argument('--cold-draw', type=int, default=0, metavar='D',
                   help='--cold-start: which draw of the kept subsets (default 0); another D gives another split')
    p.add_argument('--shortlist', type=int, default=None, metavar='M',
                   help='--recommend / --rank-eval / --explain of the recommended pairs: score only every user\'s M unseen items '
                        'with the most co-rating votes ("people who liked what you liked also liked", counted on the device) '
                        'instead of all of them; --rank-eval counts a held-out item the shortlist cut as a miss and also writes '
                        'the shortlist\'s own recall.  A user without ratings gets its M lowest unseen item ids.  Not with '
                        '--rank-negatives')
    p.add_argument('--shortlist-min-rating', type=float, default=None, metavar='X',
                   help='--shortlist: only ratings >= X count, as what a user liked and as a vote (default: every rating)')
    p.add_argument('--new-ratings', default=None, metavar='FILE',
                   help='rating changes applied to the training graph ON THE DEVICE before --recommend / --rank-eval: lines '
                        '"user item rating" (ids as recommendations_*.tsv prints them, "#" comments; rating 0 removes the '
                        'entry, ids beyond the graph create new users / items).  Takes no --use-features: the command line '
                        'cannot name a new node\'s feature rows (recommend.GraphView(dataset, graph, u_features, v_features) '
                        'can)')
    p.add_argument('--explain', type=int, default=0, metavar='M',
                   help='write the M neighbours that move each prediction most (leave-one-out attribution on the device) and '
                        'stop; explains the links of --explain-links, or with --recommend N every recommended (user, item); '
                        '0 = off')
    p.add_argument('--explain-links', default=None, metavar='FILE',
                   help='--explain: the links to explain, lines "user item" (ids as recommendations_*.tsv prints them, "#" '
                        'comments)')
    p.add_argument('--pair-epochs', type=int, default=None, metavar='E',
                   help='after training (or after loading model_checkpoint{epochs}.pth under --no-train) and before any serving '
                        'stage, fine-tune E epochs for RANKING on the training links: every link against an unseen item of its '
                        'user drawn on the device, so that the observed one scores higher; appends to pair_log.txt, saves '
                        'pair_checkpoint{E}.pth, and the serving stages of the same command use the tuned weights')
    p.add_argument('--pair-checkpoint', type=int, default=None, metavar='E',
                   help='serving stages load pair_checkpoint{E}.pth instead of model_checkpoint{epochs}.pth (no fine-tuning)')
    p.add_argument('--pair-lr', type=float, default=None, metavar='LR', help='--pair-epochs: learning rate (default 0.1 x --lr)')
    p.add_argument('--pair-mse-weight', type=float, default=None, metavar='A',
                   help='--pair-epochs: weight of the positives\' squared error beside the pair term (default 1.0: the scores '
                        'stay ratings; 0 = the plain pairwise objective)')
    p.add_argument('--pair-shortlist', type=int, default=None, metavar='M',
                   help='--pair-epochs: HARD negatives -- a share of every epoch\'s pairs takes its negative from the user\'s M '
                        'unseen items with the most co-rating votes over the training graph (the list --shortlist M serves '
                        'from; built once on the device) instead of from the whole catalogue; the pair log then tells the two '
                        'kinds apart.  Independent of --shortlist, which shortens the serving stages\' lists')
    p.add_argument('--pair-hard-share', type=float, default=None, metavar='P',
                   help='--pair-shortlist: the share of pairs whose negative is asked of the shortlist, in [0, 1] (default 0.5: '
                        'a first value, not a tuned one)')
    p.add_argument('--pair-shortlist-min-rating', type=float, default=None, metavar='X',
                   help='--pair-shortlist: only ratings >= X count, as what a user liked and as a vote (default: every rating)')
    p.add_argument('--rank-min-rating', type=float, default=None, metavar='X',
                   help='--rank-eval: only held-out links rated >= X are relevant (default: all of them)')
    p.add_argument('--ensemble', action='store_true', default=False)
    p.add_argument('--standard-rating', action='store_true', default=False)
    # sparsity experiment settings
    p.add_argument('--ratio', type=float, default=1.0)
    return p


def rating_maps(args):
    """reference ``Main.py:153-177``."""
    rating_map, post_rating_map = None, None
    if args.standard_rating:
        if args.data_name in ['flixster', 'ml_10m']:
            rating_map = {x: int(math.ceil(x)) for x in np.arange(0.5, 5.01, 0.5).tolist()}
        elif args.data_name == 'yahoo_music':
            rating_map = {x: (x - 1) // 20 + 1 for x in range(1, 101)}
    if args.transfer:
        if args.data_name in ['flixster', 'ml_10m']:
            levels = np.arange(0.5, 5.01, 0.5).tolist()
            post_rating_map = {x: int(i // (10 / args.num_relations)) for i, x in enumerate(levels)}
        elif args.data_name == 'yahoo_music':
            levels = np.arange(1, 101).tolist()
            post_rating_map = {x: int(i // (100 / args.num_relations)) for i, x in enumerate(levels)}
        else:
            levels = np.arange(1, 6).tolist()
            post_rating_map = {x: int(i // (5 / args.num_relations)) for i, x in enumerate(levels)}
    return rating_map, post_rating_map


def recommend_users(spec, n_users):
    """``--recommend-users``: None = every user, a number K = the first K user ids, else a file with one id per line."""
    if spec is None:
        return None
    if spec.isdigit():
        return np.arange(min(int(spec), n_users), dtype=np.int32)
    with open(spec) as f:
        return np.asarray([int(line) for line in f if line.strip()], dtype=np.int32)


def shortlist_flag_error(shortlist, min_rating, rank_negatives, serving):
    """The argument error of ``--shortlist`` / ``--shortlist-min-rating`` in this combination of flags, or None."""
    if shortlist is None:
        return '--shortlist-min-rating names the ratings that count for --shortlist M: give M' if min_rating is not None else None
    if not 1 <= shortlist < 2 ** 31:
        return '--shortlist takes M in [1, 2^31)'
    if rank_negatives is not None:
        return '--shortlist and --rank-negatives exclude one another: sampled negatives are an evaluation protocol, a ' \
               'shortlist is a retrieval stage'
    if not serving:
        return '--shortlist shortens the candidate lists of --recommend N / --rank-eval K[,K...]: give one of them'
    return None


def pair_flag_error(pair_epochs, pair_checkpoint, pair_lr, pair_mse_weight, dgcnn_rs, world):
    """The argument error of ``--pair-epochs`` / ``--pair-checkpoint`` / ``--pair-lr`` / ``--pair-mse-weight`` in this combination
    of flags (``world``: the number of ranks of the job), or None."""
    if pair_epochs is None:
        if pair_lr is not None:
            return '--pair-lr names the learning rate of --pair-epochs E: give E'
        if pair_mse_weight is not None:
            return '--pair-mse-weight names the squared-error weight of --pair-epochs E: give E'
        if pair_checkpoint is not None and pair_checkpoint < 1:
            return '--pair-checkpoint takes E >= 1'
        return None
    if pair_epochs < 1:
        return '--pair-epochs takes E >= 1'
    if pair_checkpoint is not None:
        return '--pair-epochs and --pair-checkpoint exclude one another: fine-tune, or serve what a fine-tuning saved'
    if dgcnn_rs:
        return '--pair-epochs fine-tunes IGMC: not with --dgcnn-rs'
    if world > 1:
        return '--pair-epochs runs on one rank (this job has %d)' % world
    if pair_lr is not None and not pair_lr > 0:
        return '--pair-lr takes LR > 0'
    if pair_mse_weight is not None and not pair_mse_weight >= 0:
        return '--pair-mse-weight takes A >= 0'
    return None


def pair_checkpoint_path(res_dir, E):
    """Where ``--pair-epochs E`` saves and ``--pair-checkpoint E`` loads: a state dict like ``model_checkpoint{N}.pth``."""
    return os.path.join(res_dir, 'pair_checkpoint{}.pth'.format(E))


def pair_shortlist_flag_error(pair_epochs, pair_shortlist, pair_hard_share, pair_shortlist_min_rating):
    """The argument error of ``--pair-shortlist`` / ``--pair-hard-share`` / ``--pair-shortlist-min-rating`` in this combination
    of flags, or None."""
    if pair_epochs is None:
        for value, flag in ((pair_shortlist, '--pair-shortlist'), (pair_hard_share, '--pair-hard-share'),
                            (pair_shortlist_min_rating, '--pair-shortlist-min-rating')):
            if value is not None:
                return '%s shapes the negatives of --pair-epochs E: give E' % flag
        return None
    if pair_shortlist is None:
        if pair_hard_share is not None:
            return '--pair-hard-share names the share of negatives drawn from --pair-shortlist M: give M'
        if pair_shortlist_min_rating is not None:
            return '--pair-shortlist-min-rating names the ratings that count for --pair-shortlist M: give M'
        return None
    if not 1 <= pair_shortlist < 2 ** 31:
        return '--pair-shortlist takes M in [1, 2^31)'
    if pair_hard_share is not None and not 0 <= pair_hard_share <= 1:
        return '--pair-hard-share takes P in [0, 1]'
    return None


def pair_log_line(info):
    line = 'Pair epoch {}, pair loss {:.6f}, mse {:.6f}, pair acc {:.6f}'.format(info['epoch'], info['pair_loss'], info['mse'],
                                                                                info['pair_acc'])
    if 'hard_pairs' in info:          # (--pair-shortlist: the share of valid pairs with a shortlist negative, accuracy per kind)
        line += ', hard {:.6f}, pair acc hard {:.6f}, uniform {:.6f}'.format(info['hard_pairs'] / max(info['pairs'], 1),
                                                                             info['pair_acc_hard'], info['pair_acc_uniform'])
    return line + '\n'


def shortlist_min_rel(class_values, min_rating):
    """The relation index both thresholds of ``--shortlist`` take: that of the smallest ``class_values`` entry >=
    ``--shortlist-min-rating`` (their number where there is none: no rating counts); 0 without the flag."""
    if min_rating is None:
        return 0
    return int((np.asarray(class_values, np.float64) < float(min_rating)).sum())


def shortlist_kwargs(args):
    if args.shortlist is None:
        return {}
    return dict(shortlist=args.shortlist, seed_min_rel=args.shortlist_min_rel, vote_min_rel=args.shortlist_min_rel)


def write_recommendations(model, train_graphs, args):
    """``--recommend N``: ``<res_dir>/recommendations_<data_name>.tsv`` with lines ``user\trank\titem\tscore`` (ranks
    from 1, best first; a user with fewer than N unseen items has fewer lines)."""
    import time
    from igmc_amd.recommend import recommend
    users = recommend_users(args.recommend_users, train_graphs.graph.n_users)
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    items, scores, counts = recommend(model, train_graphs, users=users, n=args.recommend, batch_size=args.batch_size,
                                      stats=stats, **shortlist_kwargs(args))
    items, scores, counts = items.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy()      # (synchronises)
    dt = time.perf_counter() - t0
    ids = np.arange(train_graphs.graph.n_users) if users is None else users
    path = os.path.join(args.res_dir, 'recommendations_{}.tsv'.format(args.data_name))
    with open(path, 'w') as f:
        for u, row, srow, c in zip(ids, items, scores, counts):
            for r in range(int(c)):
                f.write('%d\t%d\t%d\t%.6f\n' % (u, r + 1, row[r], srow[r]))
    print('Recommended for {} users: {} candidates scored in {} pass(es), {:.0f} candidates/s; wrote {}'.format(
        stats['users'], stats['candidates'], stats['passes'], stats['candidates'] / max(dt, 1e-9), path) +
        ('' if args.shortlist is None else ' (shortlist {})'.format(args.shortlist)))
    # (--explain without --explain-links: the recommended pairs, in the file's order)
    args.recommended_pairs = (np.repeat(np.asarray(ids, np.int32), counts),
                              np.concatenate([row[:int(c)] for row, c in zip(items, counts)] or [np.zeros(0, np.int32)]))
    return path


def write_explanations(model, train_graphs, class_values, args):
    """``--explain M``: ``<res_dir>/explanations_<data_name>.tsv`` -- a header line, then per explained link its (up to) M
    neighbours by falling |delta| with the columns ``user item score place side node rating delta score_without``: ``score`` the
    link's prediction, ``side`` ``user`` (someone who rated the item) or ``item`` (something the user rated), ``rating`` the
    ``class_values`` entry that joins the neighbour to the opposite target or ``-``, ``delta`` = ``score_without`` - ``score``.
    A link whose targets have no neighbours gets one line with place 0 and ``-`` for side, node and rating."""
    import time
    from igmc_amd.explain import explain, read_links
    if args.explain_links:
        u, v = read_links(args.explain_links)
    else:
        u, v = args.recommended_pairs
    path = os.path.join(args.res_dir, 'explanations_{}.tsv'.format(args.data_name))
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = explain(model, train_graphs, u, v, m=args.explain, batch_size=args.batch_size, stats=stats) if len(u) else None
    res = {k: t.cpu().numpy() for k, t in res.items()} if res else None      # (synchronises)
    dt = time.perf_counter() - t0
    values = np.asarray(class_values).tolist()
    with open(path, 'w') as f:
        f.write('user\titem\tscore\tplace\tside\tnode\trating\tdelta\tscore_without\n')
        for i in range(len(u)):
            b = float(res['base'][i])
            if res['counts'][i] == 0:
                f.write('%d\t%d\t%.6f\t0\t-\t-\t-\t%.6f\t%.6f\n' % (u[i], v[i], b, 0.0, b))
            for r in range(int(res['counts'][i])):
                code, d = int(res['ratings'][i, r]), float(res['deltas'][i, r])
                f.write('%d\t%d\t%.6f\t%d\t%s\t%d\t%s\t%.6f\t%.6f\n' % (
                    u[i], v[i], b, r + 1, 'item' if res['sides'][i, r] else 'user', res['nodes'][i, r],
                    '%g' % values[code - 1] if code else '-', d, b + d))
    print('Explained {} links: {} leave-one-out variants scored in {} pass(es), {:.0f} variants/s; wrote {}'.format(
        len(u), stats.get('variants', 0), stats.get('passes', 0), stats.get('variants', 0) / max(dt, 1e-9), path))
    return path


def rank_eval_ks(spec):
    """``--rank-eval 5,10``: the cut-offs K, 1 to 8 integers >= 1."""
    try:
        ks = [int(x) for x in spec.split(',')]
    except ValueError:
        ks = []
    if not 1 <= len(ks) <= 8 or min(ks) < 1:
        raise SystemExit('--rank-eval takes 1 to 8 comma-separated cut-offs K >= 1, e.g. 5,10,20')
    return ks


def write_ranking(model, train_graphs, heldout_graphs, args):
    """``--rank-eval``: ``<res_dir>/ranking_<data_name>.tsv`` with lines ``metric\tvalue`` -- the ranking metrics of the held-out
    links among every user's unseen items of the training graph (``igmc_amd/rank_eval.py``); with ``--rank-negatives K`` among
    K sampled ones, and two more lines ``negatives\tK`` and ``draw\tD``; with ``--shortlist M`` among the user's M unseen items
    with the most co-rating votes, held-out items the shortlist cut counted as misses, and three more lines ``shortlist\tM``,
    ``cut_by_shortlist\tn`` and ``shortlist_recall\tx`` (the share of the relevant held-out candidate links the shortlist
    keeps: ``rank_eval.shortlist_recall``, micro)."""
    import time
    from igmc_amd.rank_eval import HeldOut, metric_names, rank_eval, shortlist_recall
    ks = rank_eval_ks(args.rank_eval)
    users = recommend_users(args.recommend_users, train_graphs.graph.n_users)
    heldout = HeldOut.from_links(heldout_graphs, min_rating=args.rank_min_rating)
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sampled = {} if args.rank_negatives is None else dict(negatives=args.rank_negatives, draw=args.rank_draw)
    short = shortlist_kwargs(args)
    res = rank_eval(model, train_graphs, heldout, ks=ks, batch_size=args.batch_size, users=users, stats=stats,
                    **sampled, **short)      # (synchronises)
    dt = time.perf_counter() - t0
    recall = None
    if short:
        recall = shortlist_recall(train_graphs, heldout, ms=(args.shortlist,), users=users, seed_min_rel=short['seed_min_rel'],
                                  vote_min_rel=short['vote_min_rel'])[args.shortlist]['micro']
    names = metric_names(ks)
    path = os.path.join(args.res_dir, 'ranking_{}.tsv'.format(args.data_name))
    with open(path, 'w') as f:
        for k in names:
            f.write('%s\t%.6f\n' % (k, res[k]))
        if sampled:
            f.write('negatives\t%d\ndraw\t%d\n' % (args.rank_negatives, args.rank_draw))
        if short:
            f.write('shortlist\t%d\ncut_by_shortlist\t%d\nshortlist_recall\t%.6f\n' % (args.shortlist, stats['cut_by_shortlist'],
                                                                                       recall))
    print('Ranked {} held-out links of {} users ({} not among the candidates; means over {} users) among {} candidates in '
          '{} pass(es), {:.0f} candidates/s: {}; wrote {}'.format(
              stats['queries'], stats['users'], stats['not_candidates'], res['users_evaluated'], stats['candidates'],
              stats['passes'], stats['candidates'] / max(dt, 1e-9), ', '.join('%s %.4f' % (k, res[k]) for k in names), path) +
          ('' if not short else ' (shortlist {}: {} held-out candidates cut and counted as misses, shortlist recall {:.4f})'.format(
              args.shortlist, stats['cut_by_shortlist'], recall)))
    return path


def cold_start_levels(spec):
    """``--cold-start 1,2,5``: the given levels, 1 to 8 distinct integers >= 0; None where ``spec`` is malformed."""
    try:
        levels = [int(x) for x in spec.split(',')]
    except (ValueError, AttributeError):
        return None
    if not 1 <= len(levels) <= 8 or min(levels) < 0 or len(set(levels)) != len(levels):
        return None
    return levels


def cold_start_flag_error(cold_start, cold_users, cold_draw, rank_eval, new_ratings):
    """The argument error of ``--cold-start`` / ``--cold-users`` / ``--cold-draw`` in this combination of flags, or None."""
    if cold_start is None:
        if cold_users is not None:
            return '--cold-users names the users of --cold-start K[,K...]: give its levels'
        if cold_draw:
            return '--cold-draw names the draw of --cold-start K[,K...]: give its levels'
        return None
    if cold_start_levels(cold_start) is None:
        return '--cold-start takes 1 to 8 distinct comma-separated levels K >= 0, e.g. 1,2,5,10'
    if cold_draw < 0:
        return '--cold-draw takes D >= 0'
    if not rank_eval:
        return '--cold-start ranks at the cut-offs of --rank-eval K[,K...]: give them'
    if new_ratings:
        return '--cold-start and --new-ratings exclude one another: the split removes ratings from the training graph itself'
    return None


def write_cold_start(model, train_graphs, heldout_graphs, args):
    """``--cold-start``: ``<res_dir>/coldstart_<data_name>.tsv`` with lines ``given\tblock\tmetric\tvalue`` -- ``given`` a level
    or ``full``; block ``heldout``: the removed ratings and the held-out links of the level's users ranked over the reduced
    graph, ``extra``: the same ranks with the held-out links alone counted (``full``: over the unreduced graph, what
    ``--rank-eval`` reports for those users) -- (``igmc_amd/rank_eval.py``: ``cold_start_eval`` and its two caveats)."""
    from igmc_amd.rank_eval import cold_start_eval, metric_names
    ks = rank_eval_ks(args.rank_eval)
    levels = cold_start_levels(args.cold_start)
    users = recommend_users(args.cold_users, train_graphs.graph.n_users)
    kw = shortlist_kwargs(args)
    if args.rank_negatives is not None:
        kw.update(negatives=args.rank_negatives, negatives_draw=args.rank_draw)
    stats = {}
    res = cold_start_eval(model, train_graphs, given=levels, users=users, extra=heldout_graphs, ks=ks, draw=args.cold_draw,
                          min_rating=args.rank_min_rating, stats=stats, batch_size=args.batch_size, **kw)
    names = metric_names(ks)
    path = os.path.join(args.res_dir, 'coldstart_{}.tsv'.format(args.data_name))
    with open(path, 'w') as f:
        for given in levels + ['full']:
            for block in ('heldout', 'extra'):
                if block in res[given]:
                    for k in names:
                        f.write('%s\t%s\t%s\t%.6f\n' % (given, block, k, res[given][block][k]))
    print('Cold start: {} users with more than {} ratings ({} skipped)'.format(stats['users'], max(levels), stats['users_skipped']))
    for given in levels + ['full']:
        print('Given {}: {}'.format(given, '; '.join(
            '{} (means over {} users) {}'.format(block, res[given][block]['users_evaluated'],
                                                 ', '.join('%s %.4f' % (k, res[given][block][k]) for k in names))
            for block in ('heldout', 'extra') if block in res[given])))
    print('wrote {}'.format(path))
    return path


def apply_new_ratings(train_graphs, class_values, args):
    """``--new-ratings FILE``: the training set's extraction settings over its rating graph after the file's changes
    (``engine.Graph.updated``: built on the device, the training graph itself stays as it is)."""
    import time
    from igmc_amd.new_ratings import read_new_ratings
    from igmc_amd.recommend import GraphView
    u, v, r = read_new_ratings(args.new_ratings, class_values)
    old = train_graphs.graph
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    graph = old.updated(u, v, r)          # (synchronous)
    dt = time.perf_counter() - t0
    print('Applied {} rating change(s) on the device in {:.3f} ms: {} x {} with {} ratings -> {} x {} with {}'.format(
        len(u), dt * 1e3, old.n_users, old.n_items, old.nnz, graph.n_users, graph.n_items, graph.nnz))
    return GraphView(train_graphs, graph)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    from igmc_amd.new_ratings import flag_error
    bad = flag_error(args.new_ratings, args.recommend or args.explain, args.rank_eval, args.use_features)
    if bad:
        parser.error(bad)
    if args.rank_negatives is not None and not args.rank_eval:
        parser.error('--rank-negatives samples the negatives of --rank-eval: give its cut-offs K[,K...]')
    if args.rank_negatives is not None and not 0 <= args.rank_negatives < 2 ** 31:
        parser.error('--rank-negatives takes K in [0, 2^31)')
    if args.rank_draw and args.rank_negatives is None:
        parser.error('--rank-draw names the draw of --rank-negatives K: give K')
    if args.rank_draw < 0:
        parser.error('--rank-draw takes D >= 0')
    bad = shortlist_flag_error(args.shortlist, args.shortlist_min_rating, args.rank_negatives, args.recommend > 0 or args.rank_eval)
    if bad:
        parser.error(bad)
    bad = cold_start_flag_error(args.cold_start, args.cold_users, args.cold_draw, args.rank_eval, args.new_ratings)
    if bad:
        parser.error(bad)
    if args.explain < 0 or args.explain > 64:
        parser.error('--explain takes M in [1, 64]')
    if args.explain > 0 and not args.explain_links and not args.recommend > 0:
        parser.error('--explain needs the links to explain: --explain-links FILE, or --recommend N for the recommended pairs')
    if args.explain_links and not args.explain > 0:
        parser.error('--explain-links names the links of --explain M: give M')
    bad = pair_flag_error(args.pair_epochs, args.pair_checkpoint, args.pair_lr, args.pair_mse_weight, args.dgcnn_rs,
                          int(os.environ.get('WORLD_SIZE', '1')))
    if bad:
        parser.error(bad)
    bad = pair_shortlist_flag_error(args.pair_epochs, args.pair_shortlist, args.pair_hard_share, args.pair_shortlist_min_rating)
    if bad:
        parser.error(bad)
    rank, world = parallel.init_from_env()
    torch.manual_seed(args.seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(args.seed)
    if rank == 0:
        print(args)
    random.seed(args.seed)
    np.random.seed(args.seed)
    args.hop = int(args.hop)
    if args.max_nodes_per_hop is not None:
        args.max_nodes_per_hop = int(args.max_nodes_per_hop)
    rating_map, post_rating_map = rating_maps(args)

    args.file_dir = os.getcwd()          # the reference resolves the literal '__file__' against the cwd (Main.py:183)
    val_test_appendix = 'testmode' if args.testing else 'valmode'
    args.res_dir = os.path.join(args.file_dir, 'results/{}{}_{}'.format(args.data_name, args.save_appendix,
                                                                        val_test_appendix))
    src_dir = args.res_dir if args.transfer == '' else args.transfer
    args.model_pos = os.path.join(src_dir, 'model_checkpoint{}.pth'.format(args.epochs))
    if rank == 0:
        os.makedirs(args.res_dir, exist_ok=True)
        with open(os.path.join(args.res_dir, 'cmd_input.txt'), 'a') as f:
            f.write('python ' + ' '.join(sys.argv) + '\n')
    parallel.barrier()

    def logger(info, model, optimizer):
        """reference ``Main.py:31-45``."""
        epoch, train_loss, test_rmse = info['epoch'], info['train_loss'], info['test_rmse']
        with open(os.path.join(args.res_dir, 'log.txt'), 'a') as f:
            f.write('Epoch {}, train loss {:.4f}, test rmse {:.6f}\n'.format(epoch, train_loss, test_rmse))
        if type(epoch) == int and epoch % args.save_interval == 0:
            print('Saving model states...')
            if model is not None:
                torch.save(model.state_dict(), os.path.join(args.res_dir, 'model_checkpoint{}.pth'.format(epoch)))
            if optimizer is not None:
                torch.save(optimizer.state_dict(),
                           os.path.join(args.res_dir, 'optimizer_checkpoint{}.pth'.format(epoch)))

    # ---- data (reference Main.py:228-251)
    if args.data_name in ['flixster', 'douban', 'yahoo_music']:
        split = load_data_monti(args.data_name, args.testing, rating_map, post_rating_map)
    elif args.data_name == 'ml_100k':       # reference Main.py:236-243: the official u1.base / u1.test split
        if rank == 0:
            print('Using official MovieLens split u1.base/u1.test with 20% validation...')
        split = load_official_trainvaltest_split(args.data_name, args.testing, rating_map, post_rating_map, args.ratio,
                                                 verbose=(rank == 0))
    else:
        split = create_trainvaltest_split(args.data_name, args.data_seed, args.testing, None, True, rank == 0,
                                          rating_map, post_rating_map, args.ratio)
    (u_features, v_features, adj_train, train_labels, train_u, train_v, val_labels, val_u, val_v,
     test_labels, test_u, test_v, class_values) = split
    if rank == 0:
        print('All ratings are:')
        print(class_values)
    args.shortlist_min_rel = shortlist_min_rel(class_values, args.shortlist_min_rating)
    if args.use_features:
        if u_features is None or v_features is None:
            raise ValueError('--use-features: dataset %s has no side features here' % args.data_name)
        u_features, v_features = u_features.toarray(), v_features.toarray()
        n_features = u_features.shape[1] + v_features.shape[1]
    else:
        u_features, v_features, n_features = None, None, 0
    if args.debug:
        num_data = 1000
        train_u, train_v, train_labels = train_u[:num_data], train_v[:num_data], train_labels[:num_data]
        val_u, val_v, val_labels = val_u[:num_data], val_v[:num_data], val_labels[:num_data]
        test_u, test_v, test_labels = test_u[:num_data], test_v[:num_data], test_labels[:num_data]
    if rank == 0:
        print('#train: %d, #val: %d, #test: %d' % (len(train_u), len(val_u), len(test_u)))

    # ---- datasets (reference Main.py:297-350): GPU-resident; static datasets keep their node sets under
    #      data/<name>/<mode>/<part>/processed/ (MyDataset.process: built by rank 0, loaded by the others)
    data_combo = (args.data_name, args.data_appendix, val_test_appendix)
    if args.reprocess:
        if rank == 0:
            for part in ('train', 'val', 'test'):
                d = 'data/{}{}/{}/{}'.format(*(data_combo + (part,)))
                if os.path.isdir(d):
                    rmtree(d)
        parallel.barrier()      # nobody looks for a cache before rank 0 has removed the old one
    if args.dgcnn_rs and args.use_features:
        raise SystemExit('--dgcnn-rs takes no side features (the sort-pool readout has no place for them, '
                         'reference models.py:123-167): drop --use-features')

    def make(dynamic, part, idx, labels, max_num):
        cls = MyDynamicDataset if dynamic else MyDataset
        return cls('data/{}{}/{}/{}'.format(*(data_combo + (part,))), adj_train, idx, labels, args.hop,
                   args.sample_ratio, args.max_nodes_per_hop, u_features, v_features, class_values,
                   max_num=max_num, seed=args.seed)

    train_graphs = make(args.dynamic_train, 'train', (train_u, train_v), train_labels, args.max_train_num)
    test_graphs = make(args.dynamic_test, 'test', (test_u, test_v), test_labels, args.max_test_num)
    if not args.testing:
        test_graphs = make(args.dynamic_val, 'val', (val_u, val_v), val_labels, args.max_val_num)
    if rank == 0:
        print('Used #train graphs: %d, #test graphs: %d' % (len(train_graphs), len(test_graphs)))

    # ---- model (reference Main.py:381-402)
    if args.transfer:
        num_relations, multiply_by = args.num_relations, args.multiply_by
    else:
        num_relations, multiply_by = len(class_values), 1
    if args.dgcnn_rs:
        # the reference keeps this model behind `if False` (Main.py:364-380); --dgcnn-rs is the switch it never had
        from igmc_amd.models import DGCNN_RS
        model = DGCNN_RS(train_graphs, latent_dim=[32, 32, 32, 1], k=args.k, num_relations=len(class_values),
                         num_bases=4, regression=True, adj_dropout=args.adj_dropout,
                         force_undirected=args.force_undirected, seed=args.seed)
        if not args.transfer and rank == 0:     # record the k used in sortpooling (reference Main.py:376-380)
            with open(os.path.join(args.res_dir, 'cmd_input.txt'), 'a') as f:
                f.write(' --k ' + str(model.k) + '\n')
                print('k is saved.')
    else:
        model = IGMC(train_graphs, latent_dim=[32, 32, 32, 32], num_relations=num_relations, num_bases=4,
                     regression=True, adj_dropout=args.adj_dropout, force_undirected=args.force_undirected,
                     side_features=args.use_features, n_side_features=n_features, multiply_by=multiply_by,
                     seed=args.seed)
    if rank == 0:
        print('Total number of parameters is {}'.format(sum(p.numel() for p in model.parameters())))

    rmse = float('nan')
    if not args.no_train:
        rmse = train_multiple_epochs(train_graphs, test_graphs, model, args.epochs, args.batch_size, args.lr,
                                     lr_decay_factor=args.lr_decay_factor,
                                     lr_decay_step_size=args.lr_decay_step_size, weight_decay=0, ARR=args.ARR,
                                     test_freq=args.test_freq, logger=logger, continue_from=args.continue_from,
                                     res_dir=args.res_dir)
    # only rank 0 writes checkpoints (inside `logger`): nobody may look for them before it is done
    parallel.barrier()

    if args.pair_epochs:
        # no reference counterpart: E epochs of pairwise fine-tuning on the training links (igmc_amd/pair_train.py); what
        # follows -- the serving stages, the final test -- loads the tuned weights
        from igmc_amd.pair_train import train_pairs
        if args.no_train:
            model.load_state_dict(torch.load(args.model_pos, map_location='cpu'))

        def pair_logger(info):
            with open(os.path.join(args.res_dir, 'pair_log.txt'), 'a') as f:
                f.write(pair_log_line(info))

        hard = {}
        if args.pair_shortlist is not None:          # (the table is over train_graphs' rating graph: before --new-ratings)
            min_rel = shortlist_min_rel(class_values, args.pair_shortlist_min_rating)
            hard = dict(shortlist=args.pair_shortlist, hard_share=0.5 if args.pair_hard_share is None else args.pair_hard_share,
                        seed_min_rel=min_rel, vote_min_rel=min_rel)
        train_pairs(model, train_graphs, args.pair_epochs, args.batch_size,
                    0.1 * args.lr if args.pair_lr is None else args.pair_lr,
                    mse_weight=1.0 if args.pair_mse_weight is None else args.pair_mse_weight, ARR=args.ARR, logger=pair_logger,
                    **hard)
        args.model_pos = pair_checkpoint_path(args.res_dir, args.pair_epochs)
        torch.save(model.state_dict(), args.model_pos)
        print('Saved pair-tuned model states to {}'.format(os.path.basename(args.model_pos)))
    elif args.pair_checkpoint is not None:
        args.model_pos = pair_checkpoint_path(args.res_dir, args.pair_checkpoint)
        if rank == 0:
            print('Serving from {}'.format(os.path.basename(args.model_pos)))

    if args.recommend > 0 or args.rank_eval or args.explain > 0:
        # no reference counterpart: the checkpoint's N best unseen items per user over adj_train, with the training set's
        # extraction settings, and / or why it predicts what it predicts for given links (--explain: the neighbours whose
        # removal moves the score most), and / or where the held-out links (test split under --testing, else validation split) stand
        # among those items (and nothing else of what follows).  Rank 0 does the work; the other ranks wait at the barrier.
        if args.rank_eval:
            rank_eval_ks(args.rank_eval)
        model.load_state_dict(torch.load(args.model_pos, map_location='cpu'))
        if rank == 0:
            over = apply_new_ratings(train_graphs, class_values, args) if args.new_ratings else train_graphs
            if args.recommend > 0:
                write_recommendations(model, over, args)
            if args.rank_eval and args.cold_start:
                write_cold_start(model, over, test_graphs, args)
            elif args.rank_eval:
                write_ranking(model, over, test_graphs, args)
            if args.explain > 0:
                write_explanations(model, over, class_values, args)
        parallel.barrier()
        return rmse

    if args.visualize:
        # reference Main.py:423-435: the checkpoint's highest / lowest scored test subgraphs as a PDF (and nothing else of
        # what follows).  Rank 0 scores the whole test set and draws; the other ranks wait at the barrier.
        model.load_state_dict(torch.load(args.model_pos, map_location='cpu'))
        if rank == 0:
            visualize(model, test_graphs, args.res_dir, args.data_name, class_values, sort_by='prediction')
        parallel.barrier()
        if args.transfer:
            rmse = test_once(test_graphs, model, args.batch_size, logger)
            if rank == 0:
                print('Transfer learning rmse is: {:.6f}'.format(rmse))
        return rmse

    epoch_info = 'epoch {}'.format(args.epochs)
    if args.ensemble:
        if args.data_name == 'ml_1m':
            start_epoch, end_epoch, interval = args.epochs - 15, args.epochs, 5
        else:
            start_epoch, end_epoch, interval = args.epochs - 30, args.epochs, 10
        ckpt_dir = args.transfer if args.transfer else args.res_dir
        checkpoints = [os.path.join(ckpt_dir, 'model_checkpoint%d.pth' % x)
                       for x in range(start_epoch, end_epoch + 1, interval)]
        # rank 0 decides which of the scheduled checkpoints exist and every rank uses ITS list (a rank looking at
        # the file system on its own could ensemble a different set and all-reduce inconsistent squared errors)
        present = parallel.broadcast_object([os.path.exists(c) for c in checkpoints] if rank == 0 else None)
        missing = [c for c, ok in zip(checkpoints, present) if not ok]
        if missing:      # the reference's fixed schedule assumes its default epoch counts (Main.py:437-441)
            if rank == 0:
                print('ensemble: skipping %d missing checkpoint(s): %s' % (len(missing), ', '.join(map(os.path.basename, missing))))
            checkpoints = [c for c, ok in zip(checkpoints, present) if ok]
            if not checkpoints:
                raise FileNotFoundError('--ensemble: none of the scheduled checkpoints exist in %s' % ckpt_dir)
        epoch_info = ('transfer {}, '.format(args.transfer) if args.transfer else '') + \
            'ensemble of range({}, {}, {})'.format(start_epoch, end_epoch, interval)
        rmse = test_once(test_graphs, model, args.batch_size, logger=None, ensemble=True, checkpoints=checkpoints)
        if rank == 0:
            print('Ensemble test rmse is: {:.6f}'.format(rmse))
    elif args.transfer:
        model.load_state_dict(torch.load(args.model_pos, map_location='cpu'))
        rmse = test_once(test_graphs, model, args.batch_size, logger=None)
        epoch_info = 'transfer {}, epoch {}'.format(args.transfer, args.epochs)
    elif args.no_train:
        model.load_state_dict(torch.load(args.model_pos, map_location='cpu'))
        rmse = test_once(test_graphs, model, args.batch_size, logger=None)
    if rank == 0:
        print('Test rmse is: {:.6f}'.format(rmse))
        logger({'epoch': epoch_info, 'train_loss': 0, 'test_rmse': rmse}, None, None)
    return rmse


if __name__ == '__main__':
    main()
