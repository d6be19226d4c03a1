"""What hard pair negatives -- a share of every epoch's negatives drawn from the user's co-rating shortlist -- do to the ranking
metrics, beside uniform pair tuning and the regression checkpoint (writes ``profiles/pair_hard_<config>.txt``, command line
included):

    python tools/pair_hard_bench.py [--config douban] [--epochs 80] [--pair-epochs 5] [--shortlist 200] [--users N]

The checkpoint and every number of the table come through ``Main.py`` itself, as in ``tools/pair_bench.py``: per model
``--rank-eval 10`` over every unseen item, behind ``--shortlist M`` serving and with ``--rank-negatives 99``, and the test RMSE;
the tuning runs' own ``Pair epoch`` lines carry the per-kind pair accuracies.  Then, in this process on the same training graph,
medians of alternating repeats: the one-off table build (``PairLinks.set_shortlist``), one ``redraw`` through
``igmc_pair_negatives_shortlist`` and one through ``igmc_pair_negatives``.  Nothing is tuned and no number has a threshold: the
file says what the sampler does to the numbers, whichever way they move.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from pair_bench import last, main_py          # noqa: E402

KEYS = ('hr@10', 'ndcg@10', 'mrr')


def ranking(a, cwd):
    with open(os.path.join(cwd, 'results', '%s_pair_testmode' % a.config, 'ranking_%s.tsv' % a.config)) as f:
        vals = dict(l.split('\t') for l in f.read().splitlines())
    return '  '.join('%s %s' % (k, vals[k][:6]) for k in KEYS)


def measure(a, cwd, L, name, load, rmse):
    """The three protocols of the model ``load`` names (``[]``: the regression checkpoint) and its test RMSE."""
    users = [] if a.users <= 0 else ['--recommend-users', str(a.users)]
    for what, extra in (('every unseen item', []), ('--shortlist %d serving' % a.shortlist, ['--shortlist', str(a.shortlist)]),
                        ('99 sampled negatives', ['--rank-negatives', '99'])):
        main_py(a, ['--no-train'] + load + ['--rank-eval', '10'] + extra + users, cwd)
        L.append('  %-34s %-22s %s' % (name, what, ranking(a, cwd)))
        name = ''
    L.append('  %-34s test rmse %s' % ('', rmse))


def timings(a, L, repeats):
    import torch
    from igmc_amd import preprocessing
    from igmc_amd.pair_train import PairLinks
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, trl, tru, trv, _, _, _, _, _, _, cv) = preprocessing.load_data_monti(a.config, testing=True)
    ds = MyDynamicDataset('data/t/pair_hard_bench', adj, (tru, trv), trl, 1, 1.0, 200, None, None, cv, seed=1)
    pl = PairLinks(ds)

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    pl.set_shortlist(a.shortlist)          # (warm: scratch and link buffers of the first call)
    pl.redraw(1, hard_share=0.5)
    pl.redraw(1)
    build, hard, full, plain = [], [], [], []
    for r in range(repeats):          # alternating: no leg has the clocks or the caches to itself
        build.append(clock(lambda: pl.set_shortlist(a.shortlist)))
        hard.append(clock(lambda: pl.redraw(r + 2, hard_share=0.5)))
        plain.append(clock(lambda: pl.redraw(r + 2)))
        full.append(clock(lambda: pl.redraw(r + 2, hard_share=1.0)))
    labels = pl.link_y[1::2]
    L.append('')
    L.append('Sampler timings on the %s training graph (%d users x %d items, %d positives), wall clock around a synchronised '
             'call, medians of %d alternating repeats:' % (a.config, adj.shape[0], adj.shape[1], pl.n_pairs, repeats))
    L.append('  table build, M = %d (one-off; %d entries)        %.3f ms   (%s)'
             % (a.shortlist, pl.sl_total, statistics.median(build), ' '.join('%.3f' % x for x in build)))
    for name, xs in (('redraw, igmc_pair_negatives_shortlist, share 0.5', hard), ('redraw, igmc_pair_negatives_shortlist, share 1.0', full),
                     ('redraw, igmc_pair_negatives (the uniform sampler)', plain)):
        L.append('  %-52s %.3f ms   (%s)' % (name, statistics.median(xs), ' '.join('%.3f' % x for x in xs)))
    L.append('  last share-1.0 draw: %d of %d negatives from the shortlist, error word %d'
             % (int((labels == 2).sum().item()), pl.n_pairs, int(pl.err.item())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='douban', help='douban (default), flixster, yahoo_music')
    ap.add_argument('--epochs', type=int, default=80, help='epochs of the regression checkpoint trained here')
    ap.add_argument('--pair-epochs', type=int, default=5)
    ap.add_argument('--shortlist', type=int, default=200, help='M of the training table and of the --shortlist serving column')
    ap.add_argument('--users', type=int, default=0, help='rank the first N users only (0: all)')
    ap.add_argument('--repeats', type=int, default=5, help='alternating repeats of the timings (at least 3)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out_path = a.out or os.path.join(ROOT, 'profiles', 'pair_hard_%s.txt' % a.config)
    cwd = os.path.join(ROOT, 'data', 'pairbench_run')
    os.makedirs(cwd, exist_ok=True)          # (Main.py writes results/ and data/ under its working directory)
    L = ['Hard pair negatives from the co-rating shortlist, ranking before and after: one MI355X, tools/pair_hard_bench.py.',
         'command line: python tools/pair_hard_bench.py ' + ' '.join(sys.argv[1:]), '']
    t0 = time.perf_counter()
    cmd, out = main_py(a, [], cwd)
    L.append('checkpoint: %s   (%.0f s)' % (cmd, time.perf_counter() - t0))
    L.append('')
    L.append('Main.py --no-train --rank-eval 10%s [--shortlist %d | --rank-negatives 99], and the test RMSE of the same weights:'
             % ('' if a.users <= 0 else ' --recommend-users %d' % a.users, a.shortlist))
    measure(a, cwd, L, 'regression checkpoint', [], last(out, r'Test rmse is: ([0-9.]+)'))
    rows = [('uniform', [])] + [('shortlist %d, share %g' % (a.shortlist, p), ['--pair-shortlist', str(a.shortlist),
                                                                               '--pair-hard-share', '%g' % p]) for p in (0.5, 1.0)]
    for name, hard in rows:
        for A in (1.0, 0.0):
            t0 = time.perf_counter()
            cmd, out = main_py(a, ['--no-train', '--pair-epochs', str(a.pair_epochs), '--pair-mse-weight', '%g' % A] + hard, cwd)
            L.append('')
            L.append('%s   (%.0f s)' % (cmd, time.perf_counter() - t0))
            L += ['    ' + l for l in out.splitlines() if l.startswith('Pair epoch') or l.startswith('Pair training')]
            measure(a, cwd, L, '%s, A = %g' % (name, A), ['--pair-checkpoint', str(a.pair_epochs)],
                    last(out, r'Test rmse is: ([0-9.]+)'))
    timings(a, L, max(3, a.repeats))
    text = '\n'.join(L) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
