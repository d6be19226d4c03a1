"""What ranking among K sampled negatives costs beside the exhaustive evaluation (writes
``profiles/sampled_rank_eval_timing.txt``):

    python tools/sampled_rank_eval_timing.py [--negatives 99] [--users N] [--reps 3] [--warmup 1] [--out FILE]

douban, hop 1, cap 100, batch 50, every user with a test link (``--users N``: the first N of them) and their test links as
the held-out set.  Every window is warm and ends in a device synchronise; the two evaluations ALTERNATE in one process:

* ``rank_eval`` exhaustive and ``rank_eval(negatives=K)``, end to end, and the candidates per second of both -- the
  expectation: the same rate (the same pipeline), fewer links;
* HIP events (``igmc_profile_fetch``) around ``igmc_candidates_sample_count`` / ``_fill`` beside ``igmc_candidates_count`` /
  ``_fill`` on the same users -- the exhaustive enumeration is the yardstick: the sampled fill marks the same rows, walks one
  histogram more and writes far fewer links;
* the same four launches once on a synthetic graph of 40 000 items (three bitmap tiles: every walk of the sampled kernel goes
  over the tiles and rebuilds their ballots).
"""
import argparse
import contextlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from igmc_amd.hostcpu import limit_host_threads  # noqa: E402
limit_host_threads()
import numpy as np  # noqa: E402
import scipy.sparse as ssp  # noqa: E402
import torch  # noqa: E402
from igmc_amd import _lib, engine, preprocessing  # noqa: E402
from igmc_amd.models import IGMC  # noqa: E402
from igmc_amd.rank_eval import HeldOut, rank_eval  # noqa: E402
from igmc_amd.recommend import CandidateLinks  # noqa: E402
from igmc_amd.util_functions import MyDynamicDataset  # noqa: E402

KERNELS = ('k_candidates_count', 'k_candidates_fill', 'k_sampled_candidates_count', 'k_sampled_candidates_fill')


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(ms):
    return ', '.join('%.1f' % x for x in ms)


def kernel_times(lib, fn, reps):
    """us per launch of the enumeration kernels, HIP events around each: {name: [one value per repeat]}."""
    fn()
    torch.cuda.synchronize()
    lib.igmc_profile_enable(1)
    prof = {}
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
        for name, ms, calls in engine.profile_fetch(lib):          # (the fetch empties the record: one entry per repeat)
            prof.setdefault(name, []).append(ms / max(calls, 1) * 1e3)
    lib.igmc_profile_enable(0)
    return {k: v for k, v in prof.items() if k in KERNELS}


def kernel_lines(prof):
    return ['  %-28s %9.2f   (%.2f .. %.2f)' % (k, statistics.median(prof[k]), min(prof[k]), max(prof[k])) for k in KERNELS
            if k in prof]


def enumerations(source, users, negatives, must):
    """One exhaustive and one sampled refill of lists of their own (count + fill each)."""
    full = CandidateLinks.for_users(source, users)
    few = CandidateLinks.for_users(source, users, negatives=negatives, must=must)

    def run():
        full.refill(users)
        few.refill(users, negatives=negatives, must=must)
    return run, len(full), len(few)


class _Synthetic(object):
    """As much of a dataset as ``CandidateLinks`` reads, over a random graph of ``n_items`` items."""
    u_features = v_features = _side = None

    def __init__(self, like, n_users, n_items, per_row, seed):
        rng = np.random.default_rng(seed)
        rows = np.repeat(np.arange(n_users), per_row)
        cols = rng.integers(0, n_items, n_users * per_row)
        A = ssp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_users, n_items))
        A.data[:] = 1 + np.arange(A.nnz) % 5
        self.graph = engine.Graph(A, device=like.graph.device, lib=like.graph.lib)
        self.device, self.h, self.sample_ratio, self.seed = like.device, like.h, like.sample_ratio, like.seed
        self.max_nodes_per_hop, self.link_y = like.max_nodes_per_hop, like.link_y[:0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--negatives', type=int, default=99)
    ap.add_argument('--users', type=int, default=0, help='the first N users with a test link (0: all of them)')
    ap.add_argument('--mnph', type=int, default=100)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sampled_rank_eval_timing.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sampled_rank_eval_timing.py measures on the GPU: no device found')
    with contextlib.redirect_stdout(sys.stderr):
        split = preprocessing.load_data_monti('douban', testing=True)
    (_, _, adj, trl, tru, trv, _, _, _, _, teu, tev, cv) = split
    train = MyDynamicDataset('data/sampledtiming/train', adj, (tru, trv), trl, 1, 1.0, a.mnph, None, None, cv, seed=1)
    heldout = HeldOut.from_links(train, np.asarray(teu), np.asarray(tev))
    users = heldout.users if a.users <= 0 else heldout.users[:a.users]
    torch.manual_seed(1)
    model = IGMC(train, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True, adj_dropout=0.0,
                 seed=1).to('cuda')
    model.reset_parameters()
    model.eval()
    ks = (5, 10, 20)
    st_full, st_few = {}, {}
    # (lists of their own: the two evaluations would otherwise refill -- and size -- one kept list in turn)
    other = MyDynamicDataset('data/sampledtiming/train', adj, (tru, trv), trl, 1, 1.0, a.mnph, None, None, cv, seed=1)
    run_full = lambda: rank_eval(model, train, heldout, ks=ks, users=users, stats=st_full)
    run_few = lambda: rank_eval(model, other, heldout, ks=ks, users=users, stats=st_few, negatives=a.negatives)
    for _ in range(a.warmup):
        run_full()
        run_few()
    ms_full, ms_few = [], []
    for _ in range(a.reps):            # alternating: whatever else the host does hits both
        ms_full.append(timed(run_full)[0])
        ms_few.append(timed(run_few)[0])
    res_full, res_few = run_full(), run_few()
    lib = _lib.load()
    pu = res_few['per_user']
    must = (pu['offsets'], pu['items'])
    run_d, n_full_d, n_few_d = enumerations(train, pu['users'], a.negatives, must)
    prof_d = kernel_times(lib, run_d, max(a.reps, 5))
    syn = _Synthetic(train, 1000, 40000, 120, 5)
    syn_users = torch.arange(1000, dtype=torch.int32, device='cuda')
    run_s, n_full_s, n_few_s = enumerations(syn, syn_users, a.negatives, None)
    prof_s = kernel_times(lib, run_s, max(a.reps, 5))
    med_full, med_few = statistics.median(ms_full), statistics.median(ms_few)
    L = []
    L.append('Held-out ranking among %d sampled negatives beside the exhaustive evaluation: one MI355X, one process, '
             'tools/sampled_rank_eval_timing.py.' % a.negatives)
    L.append('Shape: douban (3000 x 3000), hop 1, cap %d, batch 50, %d users with a test link, %d held-out links, cut-offs %s.'
             % (a.mnph, st_full['users'], st_full['queries'], ', '.join(map(str, ks))))
    L.append('Every timed window is warm (%d calls of each before it), ends in a device synchronise inside the clock, and the two'
             % a.warmup)
    L.append('alternate (exhaustive, sampled, exhaustive, ...).')
    L.append('')
    L.append('exhaustive  rank_eval(), ms per call:               ' + fmt(ms_full))
    L.append('sampled     rank_eval(negatives=%d), ms per call:   ' % a.negatives + fmt(ms_few))
    L.append('')
    for name, med, st in (('exhaustive', med_full, st_full), ('sampled', med_few, st_few)):
        L.append('median %-10s %10.1f ms   %9d candidates in %d pass(es)   %.3f M candidates/s'
                 % (name, med, st['candidates'], st['passes'], st['candidates'] / med / 1e3))
    L.append('the sampled call takes %.1f x less time over %.1f x fewer links'
             % (med_full / med_few, st_full['candidates'] / st_few['candidates']))
    L.append('')
    L.append('the enumeration launches by themselves (HIP events around each launch, igmc_profile_fetch), us, median (min .. max):')
    L.append(' douban, the same %d users: %d links exhaustive, %d sampled (must items: the held-out links)'
             % (pu['users'].numel(), n_full_d, n_few_d))
    L += kernel_lines(prof_d)
    L.append(' synthetic 1000 x 40000 graph (three tiles), 120 ratings a user, no must items: %d links exhaustive, %d sampled'
             % (n_full_s, n_few_s))
    L += kernel_lines(prof_s)
    L.append('')
    L.append('metrics (untrained weights: the figures mean nothing, the runs do): exhaustive '
             + ', '.join('%s %.4f' % (k, v) for k, v in res_full.items() if isinstance(v, float)))
    L.append('                                                                     sampled    '
             + ', '.join('%s %.4f' % (k, v) for k, v in res_few.items() if isinstance(v, float)))
    text = '\n'.join(L) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
