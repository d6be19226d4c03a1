"""What pairwise fine-tuning does to the ranking metrics (writes ``profiles/pair_<config>.txt``, command line included):

    python tools/pair_bench.py [--config douban] [--epochs 80] [--pair-epochs 5] [--users N]

A bundled dataset and a checkpoint trained here by ``Main.py`` with the reference recipe (``--epochs``; the README recipe is 80).
Recorded, every number through ``Main.py`` itself: the checkpoint's ``--rank-eval 5,10,20`` over every unseen item and with
``--rank-negatives 99`` -- the baseline, code this feature does not touch --; both again after ``--pair-epochs E`` for
``--pair-mse-weight`` 0 and 1; the test RMSE of each model; the pair steps per second.  Nothing is tuned here: the file says
what the objective does to the numbers, whichever way they move.
"""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('hr@5', 'hr@10', 'hr@20', 'ndcg@5', 'ndcg@10', 'ndcg@20', 'mrr')


def main_py(a, extra, cwd):
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', a.config, '--epochs', str(a.epochs), '--testing',
           '--lr-decay-step-size', '50', '--save-appendix', '_pair', '--save-interval', str(a.epochs)] + extra
    p = subprocess.Popen(cmd, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True)
    out = []
    for line in p.stdout:          # (passed on as it comes: a long run shows its progress)
        out.append(line)
        sys.stderr.write(line)
        sys.stderr.flush()
    if p.wait() != 0:
        raise SystemExit('%s failed:\n%s' % (' '.join(cmd), ''.join(out)[-3000:]))
    return 'python ' + ' '.join(['Main.py'] + cmd[2:]), ''.join(out)


def last(out, pattern):
    found = re.findall(pattern, out)
    return found[-1] if found else '?'


def ranking(a, cwd):
    with open(os.path.join(cwd, 'results', '%s_pair_testmode' % a.config, 'ranking_%s.tsv' % a.config)) as f:
        vals = dict(l.split('\t') for l in f.read().splitlines())
    return '  '.join('%s %s' % (k, vals[k][:6]) for k in KEYS)


def measure(a, cwd, L, name, load):
    """The two protocols and the test RMSE of the model ``load`` names (``[]``: the regression checkpoint)."""
    users = [] if a.users <= 0 else ['--recommend-users', str(a.users)]
    main_py(a, ['--no-train'] + load + ['--rank-eval', '5,10,20'] + users, cwd)
    L.append('  %-22s every unseen item   %s' % (name, ranking(a, cwd)))
    main_py(a, ['--no-train'] + load + ['--rank-eval', '5,10,20', '--rank-negatives', '99'] + users, cwd)
    L.append('  %-22s 99 sampled negatives %s' % ('', ranking(a, cwd)))
    _, out = main_py(a, ['--no-train'] + load, cwd)
    L.append('  %-22s test rmse %s' % ('', last(out, r'Test rmse is: ([0-9.]+)')))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='douban', help='douban (default), flixster, yahoo_music')
    ap.add_argument('--epochs', type=int, default=80, help='epochs of the regression checkpoint trained here')
    ap.add_argument('--pair-epochs', type=int, default=5)
    ap.add_argument('--users', type=int, default=0, help='rank the first N users only (0: all)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out_path = a.out or os.path.join(ROOT, 'profiles', 'pair_%s.txt' % a.config)
    cwd = os.path.join(ROOT, 'data', 'pairbench_run')
    os.makedirs(cwd, exist_ok=True)          # (Main.py writes results/ and data/ under its working directory)
    L = ['Pairwise fine-tuning, ranking before and after: one MI355X, tools/pair_bench.py.',
         'command line: python tools/pair_bench.py ' + ' '.join(sys.argv[1:]), '']
    t0 = time.perf_counter()
    cmd, out = main_py(a, [], cwd)
    L.append('checkpoint: %s   (%.0f s)' % (cmd, time.perf_counter() - t0))
    L.append('')
    L.append('Main.py --no-train --rank-eval 5,10,20%s [--rank-negatives 99], and the test RMSE of the same weights:'
             % ('' if a.users <= 0 else ' --recommend-users %d' % a.users))
    measure(a, cwd, L, 'regression checkpoint', [])
    for A in (0.0, 1.0):
        t0 = time.perf_counter()
        cmd, out = main_py(a, ['--no-train', '--pair-epochs', str(a.pair_epochs), '--pair-mse-weight', '%g' % A], cwd)
        L.append('')
        L.append('%s   (%.0f s)' % (cmd, time.perf_counter() - t0))
        L += ['    ' + l for l in out.splitlines() if l.startswith('Pair epoch') or l.startswith('Pair training')]
        measure(a, cwd, L, '--pair-mse-weight %g' % A, ['--pair-checkpoint', str(a.pair_epochs)])
    text = '\n'.join(L) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
