"""What a co-rating shortlist costs and what it keeps (writes ``profiles/shortlist_<config>.txt``, command line included):

    python tools/shortlist_bench.py throughput [--config ml_1m] [--users N] [--reps 3] [--warmup 1]
    python tools/shortlist_bench.py quality    [--config douban] [--epochs 80] [--users N]

``throughput``: the ml_1m-shaped synthetic graph (``preprocessing.create_trainvaltest_split``), hop 1, cap 100, batch 50, an
untrained model (the scoring pass costs the same whatever the weights).  Per M in 100, 200, 500: the time of ONE refill of the
shortlists of all users (``igmc_candidates_count`` + ``igmc_shortlist_fill``, a device synchronise inside the clock), and the
end-to-end time of ``recommend(n=10)`` exhaustive and with each M -- every window warm, the variants ALTERNATING in one process,
medians.  The exhaustive path is code the shortlist does not touch: it stands for what the project did before.

``quality``: a bundled dataset and a checkpoint trained here by ``Main.py`` (``--epochs``; the README recipe is 80).
``rank_eval.shortlist_recall`` of the test links for M in 50, 100, 200, 500 (no model), and ``Main.py --rank-eval 5,10,20``
exhaustive and with ``--shortlist M`` side by side, with ``cut_by_shortlist``.  The synthetic MovieLens ratings are i.i.d.: only
the bundled real datasets say anything about quality.
"""
import argparse
import contextlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from igmc_amd.hostcpu import limit_host_threads  # noqa: E402
limit_host_threads()
import numpy as np  # noqa: E402
import torch  # noqa: E402
from igmc_amd import preprocessing  # noqa: E402
from igmc_amd.models import IGMC  # noqa: E402
from igmc_amd.rank_eval import HeldOut, shortlist_recall  # noqa: E402
from igmc_amd.recommend import CandidateLinks, recommend  # noqa: E402
from igmc_amd.util_functions import MyDynamicDataset  # noqa: E402

MS_THROUGHPUT = (100, 200, 500)
MS_QUALITY = (50, 100, 200, 500)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(ms):
    return ', '.join('%.1f' % x for x in ms)


def throughput(a, L):
    with contextlib.redirect_stdout(sys.stderr):
        split = preprocessing.create_trainvaltest_split(a.config, 1234, True, verbose=False)
    (_, _, adj, trl, tru, trv, _, _, _, _, _, _, cv) = split

    def dataset():
        return MyDynamicDataset('data/shortlistbench/%s' % a.config, adj, (tru, trv), trl, 1, 1.0, 100, None, None, cv, seed=1)
    # (a dataset per variant: each keeps its own candidate list and captured scoring graph, sized for its own passes)
    sets = {m: dataset() for m in (None,) + MS_THROUGHPUT}
    g = sets[None].graph
    info = g.info()
    n_users = g.n_users if a.users <= 0 else min(a.users, g.n_users)
    users = torch.arange(n_users, dtype=torch.int32, device='cuda')
    torch.manual_seed(1)
    model = IGMC(sets[None], latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True, adj_dropout=0.0,
                 seed=1).to('cuda')
    model.reset_parameters()
    model.eval()
    L.append('Shape: %s-shaped synthetic graph, %d x %d, %d ratings, max_deg_u %d, max_deg_v %d; hop 1, cap 100, batch 50; %d users.'
             % (a.config, g.n_users, g.n_items, info['nnz'], info['max_deg_u'], info['max_deg_v'], n_users))
    L.append('Every timed window is warm (%d calls before it) and ends in a device synchronise inside the clock; the variants'
             % a.warmup)
    L.append('alternate in one process; medians of %d.' % a.reps)
    L.append('')
    # ---- the refill alone
    lists = {m: CandidateLinks.for_users(sets[m], users, shortlist=m) for m in MS_THROUGHPUT}
    fill = {m: [] for m in MS_THROUGHPUT}
    for r in range(a.warmup + max(a.reps, 5)):
        for m in MS_THROUGHPUT:
            ms = timed(lambda: lists[m].refill(users, shortlist=m))[0]
            if r >= a.warmup:
                fill[m].append(ms)
    L.append('one refill of every user\'s shortlist (igmc_candidates_count + igmc_shortlist_fill + the host read of the total), ms:')
    for m in MS_THROUGHPUT:
        med = statistics.median(fill[m])
        L.append('  M = %-4d %9.2f ms a pass   %7.2f us a user   (%s)   %d links' % (m, med, med * 1e3 / n_users, fmt(fill[m]),
                                                                                 len(lists[m])))
    del lists
    # ---- recommend(n=10), end to end
    stats = {m: {} for m in sets}
    runs = {m: (lambda m=m: recommend(model, sets[m], users=users, n=10, stats=stats[m], **({} if m is None else
                                                                                             dict(shortlist=m)))) for m in sets}
    for _ in range(a.warmup):
        for m in runs:
            runs[m]()
    ms = {m: [] for m in runs}
    for _ in range(a.reps):
        for m in runs:
            ms[m].append(timed(runs[m])[0])
    L.append('')
    L.append('recommend(n=10) end to end (enumeration, scoring, top-n), ms per call:')
    med_full = statistics.median(ms[None])
    for m in runs:
        med = statistics.median(ms[m])
        L.append('  %-12s %10.1f ms   (%s)   %9d candidates in %d pass(es), %.3f M candidates/s   1 / %.1f of the exhaustive time'
                 % ('exhaustive' if m is None else 'M = %d' % m, med, fmt(ms[m]), stats[m]['candidates'], stats[m]['passes'],
                    stats[m]['candidates'] / med / 1e3, med_full / med))
    L.append('')
    L.append('enumerating a pass\'s shortlist against scoring it (the refill above against the rest of the end-to-end call):')
    for m in MS_THROUGHPUT:
        f, e = statistics.median(fill[m]), statistics.median(ms[m])
        L.append('  M = %-4d refill %.1f ms, everything else %.1f ms: the enumeration takes %s time than the scoring'
                 % (m, f, e - f, 'LESS' if f < e - f else 'MORE'))


def main_py(a, extra, cwd):
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', a.config, '--epochs', str(a.epochs), '--testing',
           '--lr-decay-step-size', '50', '--save-appendix', '_shortlist', '--save-interval', str(a.epochs)] + extra
    p = subprocess.Popen(cmd, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True)
    out = []
    for line in p.stdout:          # (passed on as it comes: a long training run shows its progress)
        out.append(line)
        sys.stderr.write(line)
        sys.stderr.flush()
    if p.wait() != 0:
        raise SystemExit('%s failed:\n%s' % (' '.join(cmd), ''.join(out)[-3000:]))
    return 'python ' + ' '.join(['Main.py'] + cmd[2:]), ''.join(out)


def quality(a, L):
    cwd = os.path.join(ROOT, 'data', 'shortlistbench_run')
    os.makedirs(cwd, exist_ok=True)          # (Main.py writes results/ and data/ under its working directory)
    t0 = time.perf_counter()
    cmd, out = main_py(a, [], cwd)
    L.append('checkpoint: %s   (%.0f s)' % (cmd, time.perf_counter() - t0))
    L += ['  ' + l for l in out.splitlines() if 'Test rmse' in l or 'test rmse' in l][-1:]
    L.append('')
    with contextlib.redirect_stdout(sys.stderr):
        split = preprocessing.load_data_monti(a.config, testing=True)
    (_, _, adj, trl, tru, trv, _, _, _, _, teu, tev, cv) = split
    train = MyDynamicDataset('data/shortlistbench/%s' % a.config, adj, (tru, trv), trl, 1, 1.0, 10000, None, None, cv, seed=1)
    heldout = HeldOut.from_links(train, np.asarray(teu), np.asarray(tev))
    users = None if a.users <= 0 else np.arange(a.users, dtype=np.int32)
    st = {}
    t, rec = timed(lambda: shortlist_recall(train, heldout, ms=MS_QUALITY, users=users, stats=st))
    L.append('shortlist_recall of the test links (no model; %d users, %d links that are candidates, %d that are not; %.1f ms for'
             % (st['users'], st['links'], st['not_candidates'], t))
    L.append('all four M, one igmc_shortlist_places pass):')
    for m in MS_QUALITY:
        L.append('  M = %-4d micro %.4f   macro %.4f' % (m, rec[m]['micro'], rec[m]['macro']))
    L.append('')
    L.append('Main.py --no-train --rank-eval 5,10,20%s, exhaustive and with --shortlist M (a held-out candidate the shortlist cut'
             % ('' if users is None else ' --recommend-users %d' % a.users))
    L.append('is a miss):')
    res_dir = os.path.join(cwd, 'results', '%s_shortlist_testmode' % a.config)
    for m in (None,) + MS_QUALITY:
        extra = ['--no-train', '--rank-eval', '5,10,20'] + ([] if users is None else ['--recommend-users', str(a.users)]) + \
            ([] if m is None else ['--shortlist', str(m)])
        main_py(a, extra, cwd)
        with open(os.path.join(res_dir, 'ranking_%s.tsv' % a.config)) as f:
            vals = dict(l.split('\t') for l in f.read().splitlines())
        L.append('  %-12s ' % ('exhaustive' if m is None else 'M = %d' % m) + '  '.join(
            '%s %s' % (k, vals[k][:6]) for k in ('hr@10', 'recall@10', 'ndcg@5', 'ndcg@10', 'ndcg@20', 'mrr')) +
            ('' if m is None else '   cut_by_shortlist %s  shortlist_recall %s' % (vals['cut_by_shortlist'], vals['shortlist_recall'])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('throughput', 'quality'))
    ap.add_argument('--config', default=None, help='throughput: ml_1m (default); quality: douban (default), flixster')
    ap.add_argument('--users', type=int, default=0, help='the first N users only (0: all)')
    ap.add_argument('--epochs', type=int, default=80, help='quality: epochs of the checkpoint trained here')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('shortlist_bench.py measures on the GPU: no device found')
    a.config = a.config or ('ml_1m' if a.what == 'throughput' else 'douban')
    out = a.out or os.path.join(ROOT, 'profiles', 'shortlist_%s.txt' % a.config)
    L = ['Co-rating shortlists, %s: one MI355X, tools/shortlist_bench.py.' % a.what,
         'command line: python tools/shortlist_bench.py ' + ' '.join(sys.argv[1:]), '']
    (throughput if a.what == 'throughput' else quality)(a, L)
    text = '\n'.join(L) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
