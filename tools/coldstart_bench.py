"""Given-k cold-start evaluation, measured: the metric table of ``Main.py --cold-start`` and the cost of the split.

    python tools/coldstart_bench.py [--config douban] [--epochs 80] [--given 1,2,5,10,20] [--out profiles/coldstart_douban.txt]

A bundled dataset and a checkpoint trained here by ``Main.py`` (``--epochs``; the README recipe is 80).  Then ``Main.py --no-train
--rank-eval 5,10,20 --cold-start <given>`` four times -- every tenth user ("a cold user in a warm system") and all users ("a cold
system"), each exhaustively and with ``--rank-negatives 99`` -- and their ``coldstart_<data>.tsv`` as one table.  Then, in this
process over the same training graph: the HIP-event time of ``igmc_holdout_fill`` for all users, and the wall time of one
level's ``rank_eval.hold_out`` (count, fill and ``engine.Graph.updated``: the reduced graph never leaves the device) against
the same split made on the host -- a numpy loop over the users' rows with a host RNG, a rebuilt scipy matrix and
``engine.Graph(A')`` uploaded --, the two interleaved, ``--warmup`` + ``--reps`` repetitions, medians.  Reported, not gated."""
import argparse
import contextlib
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as ssp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from igmc_amd import engine, preprocessing          # noqa: E402
from igmc_amd.rank_eval import hold_out          # noqa: E402
from igmc_amd.util_functions import MyDynamicDataset          # noqa: E402

KEYS = ('hr@5', 'hr@10', 'hr@20', 'ndcg@10', 'mrr')


def main_py(a, extra, cwd):
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', a.config, '--epochs', str(a.epochs), '--testing',
           '--lr-decay-step-size', '50', '--save-appendix', '_cold', '--save-interval', str(a.epochs)] + extra
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


def metric_table(a, cwd, L, n_users):
    every_tenth = os.path.join(cwd, 'every_tenth_user.txt')
    with open(every_tenth, 'w') as f:
        f.write(''.join('%d\n' % u for u in range(0, n_users, 10)))
    res_dir = os.path.join(cwd, 'results', '%s_cold_testmode' % a.config)
    for who, users in (('every tenth user (a cold user in a warm system)', ['--cold-users', every_tenth]),
                       ('all users (a cold system)', [])):
        for how, neg in (('every unseen item', []), ('99 sampled negatives', ['--rank-negatives', '99'])):
            t0 = time.perf_counter()
            _, out = main_py(a, ['--no-train', '--rank-eval', '5,10,20', '--cold-start', a.given] + users + neg, cwd)
            L.append('%s, among %s   (%.0f s; %s)' % (who, how, time.perf_counter() - t0,
                                                      ''.join(l for l in out.splitlines() if l.startswith('Cold start: '))))
            with open(os.path.join(res_dir, 'coldstart_%s.tsv' % a.config)) as f:
                vals = {tuple(l.split('\t')[:3]): l.split('\t')[3] for l in f.read().splitlines()}
            L.append('  %-6s %-8s ' % ('given', 'block') + ' '.join('%-8s' % k for k in KEYS))
            for given in a.given.split(',') + ['full']:
                for block in ('heldout', 'extra'):
                    if (given, block, KEYS[0]) in vals:
                        L.append('  %-6s %-8s ' % (given, block) + ' '.join('%-8s' % vals[(given, block, k)][:6] for k in KEYS))
            L.append('')


def host_split(A, users, keep, rng, device, lib):
    """The split the host would make: per user a random ``keep``-subset of the row stays; the reduced matrix rebuilt and uploaded."""
    indptr, stay = A.indptr, np.ones(A.nnz, bool)
    for u in users:
        lo, hi = indptr[u], indptr[u + 1]
        if hi - lo > keep:
            stay[lo:hi] = False
            stay[lo + rng.choice(hi - lo, keep, replace=False)] = True
    rows = np.repeat(np.arange(A.shape[0]), np.diff(indptr))
    B = ssp.csr_matrix((A.data[stay], (rows[stay], A.indices[stay])), shape=A.shape)
    return engine.Graph(B, device=device, lib=lib)


def timings(a, L, train):
    g = train.graph
    users = torch.arange(g.n_users, dtype=torch.int32, device=train.link_y.device)
    keep = int(a.given.split(',')[len(a.given.split(',')) // 2])
    counts, err = engine.holdout_count(g, users, keep)
    offsets = torch.zeros(g.n_users + 1, dtype=torch.int64, device=users.device)
    torch.cumsum(counts, 0, out=offsets[1:])
    total = int(offsets[-1].item())
    u, v = (torch.zeros(max(total, 1), dtype=torch.int32, device=users.device) for _ in range(2))
    r = torch.zeros(max(total, 1), dtype=torch.uint8, device=users.device)
    ev, fill = [torch.cuda.Event(enable_timing=True) for _ in range(2)], []
    for k in range(a.warmup + a.reps):
        ev[0].record()
        engine.holdout_fill(g, users, keep, None, offsets, u, v, r, err, train.seed, 0)
        ev[1].record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            fill.append(ev[0].elapsed_time(ev[1]) * 1e3)
    assert int(err.item()) == 0
    L.append('igmc_holdout_fill, all %d users of %s (%d ratings, keep %d: %d links held out), HIP events around the launch:'
             % (g.n_users, a.config, g.nnz, keep, total))
    L.append('  median %.1f us   (min %.1f, max %.1f; %d repetitions after %d warm-up)'
             % (statistics.median(fill), min(fill), max(fill), a.reps, a.warmup))
    L.append('')
    A = g.to_scipy()
    rng = np.random.default_rng(1)
    host_users = np.arange(g.n_users)
    dev_t, host_t = [], []
    for k in range(a.warmup + a.reps):          # (interleaved: both see the same machine state)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        split = hold_out(train, keep=keep)          # (ends synchronised: updated() reads the new sizes)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        hg = host_split(A, host_users, keep, rng, g.device, g.lib)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert split.graph.nnz == hg.nnz
        split.graph.close()
        hg.close()
        if k >= a.warmup:
            dev_t.append((t1 - t0) * 1e3)
            host_t.append((t2 - t1) * 1e3)
    L.append('one level\'s split, all users, keep %d, wall clock around a synchronised call (%d repetitions after %d warm-up, the two'
             % (keep, a.reps, a.warmup))
    L.append('interleaved):')
    L.append('  rank_eval.hold_out (count, fill, engine.Graph.updated on the device)   median %8.2f ms   (min %.2f, max %.2f)'
             % (statistics.median(dev_t), min(dev_t), max(dev_t)))
    L.append('  numpy split + scipy matrix + engine.Graph(A\') through the host          median %8.2f ms   (min %.2f, max %.2f)'
             % (statistics.median(host_t), min(host_t), max(host_t)))
    L.append('  ratio %.1f x' % (statistics.median(host_t) / statistics.median(dev_t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='douban', help='douban (default), flixster, yahoo_music')
    ap.add_argument('--epochs', type=int, default=80, help='epochs of the checkpoint trained here')
    ap.add_argument('--given', default='1,2,5,10,20')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-metrics', action='store_true', help='the two timings only')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('coldstart_bench.py measures on the GPU: no device found')
    out = a.out or os.path.join(ROOT, 'profiles', 'coldstart_%s.txt' % a.config)
    L = ['Given-k cold-start evaluation, %s: one MI355X, tools/coldstart_bench.py.' % a.config,
         'command line: python tools/coldstart_bench.py ' + ' '.join(sys.argv[1:]), '',
         'Blocks: heldout = the ratings the split removed AND the test links of the level\'s users, ranked over the reduced graph (the',
         'removed ratings were regression targets in training: not leak-free); extra = the same ranks, the test links alone counted',
         '(leak-free; "full": over the unreduced graph, what --rank-eval reports for those users).  Every evaluated user goes cold',
         'together.  Users with no more than max(given) training ratings are skipped.', '']
    with contextlib.redirect_stdout(sys.stderr):
        split = preprocessing.load_data_monti(a.config, testing=True)
    (_, _, adj, trl, tru, trv, _, _, _, _, teu, tev, cv) = split
    train = MyDynamicDataset('data/coldstartbench/%s' % a.config, adj, (tru, trv), trl, 1, 1.0, 10000, None, None, cv, seed=1)
    if not a.no_metrics:
        cwd = os.path.join(ROOT, 'data', 'coldstartbench_run')
        os.makedirs(cwd, exist_ok=True)          # (Main.py writes results/ and data/ under its working directory)
        t0 = time.perf_counter()
        cmd, log = main_py(a, [], cwd)
        L.append('checkpoint: %s   (%.0f s)' % (cmd, time.perf_counter() - t0))
        L += ['  ' + l for l in log.splitlines() if 'Test rmse' in l or 'test rmse' in l][-1:]
        L.append('')
        metric_table(a, cwd, L, train.graph.n_users)
    timings(a, L, train)
    text = '\n'.join(L) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
