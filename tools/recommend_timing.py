"""What a recommendation costs beside the scoring pass it is built on (writes ``profiles/recommend_scoring.txt``):

    python tools/recommend_timing.py [--users 7] [--reps 5] [--warmup 2] [--out profiles/recommend_scoring.txt]

douban, hop 1, cap 100, batch 50, a fixed set of users (the first ``--users`` ids: about 3 000 candidates each).  Three things
are timed, every window warm and ending in a device synchronise, the first two ALTERNATING in one process:

* ``score_links`` over a ``MyDynamicDataset`` built on the host from the same candidate list (numpy complement, upload) --
  the scoring pass alone; building that dataset is NOT in the window;
* ``recommend`` end to end: enumeration, the same scoring pass, selection, the gather of the items;
* the enumeration and selection kernels by themselves, HIP events around each launch (``igmc_profile_fetch``).

A breakdown of ``recommend`` (refill / score / top_n, a synchronise after each) says where its time goes.
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
from igmc_amd.recommend import recommend, score_candidates, top_n  # noqa: E402
from igmc_amd.train_eval import score_links  # noqa: E402
from igmc_amd.util_functions import MyDynamicDataset  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(ms):
    return ', '.join('%.3f' % x for x in ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=7)
    ap.add_argument('--mnph', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--n', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'recommend_scoring.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('recommend_timing.py measures on the GPU: no device found')
    with contextlib.redirect_stdout(sys.stderr):
        split = preprocessing.load_data_monti('douban', testing=True)
    (_, _, adj, trl, tru, trv, _, _, _, _, _, _, cv) = split
    A = ssp.csr_matrix(adj)
    train = MyDynamicDataset('data/rectiming/train', adj, (tru, trv), trl, 1, 1.0, a.mnph, None, None, cv, seed=1)
    users = np.arange(a.users, dtype=np.int32)
    hu, hv = [], []
    for u in users:
        keep = np.ones(A.shape[1], bool)
        keep[A.indices[A.indptr[u]:A.indptr[u + 1]]] = False
        v = np.nonzero(keep)[0]
        hu.append(np.full(len(v), u, np.int64))
        hv.append(v)
    hu, hv = np.concatenate(hu), np.concatenate(hv)
    host = MyDynamicDataset('data/rectiming/host', adj, (hu, hv), np.zeros(len(hu), np.int64), 1, 1.0, a.mnph, None, None, cv,
                            seed=1)
    torch.manual_seed(1)
    model = IGMC(train, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True, adj_dropout=0.0,
                 seed=1).to('cuda')
    model.reset_parameters()
    model.eval()
    run_a = lambda: score_links(model, host, 50)
    run_b = lambda: recommend(model, train, users=users, n=a.n)
    for _ in range(a.warmup):          # the first pass of each starts eagerly and captures its graph
        run_a()
        run_b()
    ms_a, ms_b = [], []
    for _ in range(a.reps):            # alternating: whatever else the host does hits both
        ms_a.append(timed(run_a)[0])
        ms_b.append(timed(run_b)[0])
    R = run_a()[0]
    items, scores, counts = run_b()
    cands = train._recommend_links
    same = torch.equal(score_candidates(model, cands, 50), R)
    # where recommend's time goes
    parts = {'refill': [], 'score_candidates': [], 'top_n': []}
    for _ in range(a.reps):
        parts['refill'].append(timed(lambda: cands.refill(users))[0])
        t, Rc = timed(lambda: score_candidates(model, cands, 50))
        parts['score_candidates'].append(t)
        parts['top_n'].append(timed(lambda: top_n(cands, Rc, a.n))[0])
    # the kernels by themselves
    lib = _lib.load()
    lib.igmc_profile_enable(1)
    prof = {}
    for _ in range(a.reps):
        cands.refill(users)
        top_n(cands, Rc, a.n)
        torch.cuda.synchronize()
        for name, ms, calls in engine.profile_fetch(lib):          # (the fetch empties the record: one entry per repeat)
            prof.setdefault(name, []).append(ms / max(calls, 1) * 1e3)
    lib.igmc_profile_enable(0)
    n = len(hu)
    med_a, med_b = statistics.median(ms_a), statistics.median(ms_b)
    spread_a, spread_b = max(ms_a) - min(ms_a), max(ms_b) - min(ms_b)
    inside = med_b <= med_a + spread_a
    L = []
    L.append('Cost of a recommendation beside the scoring pass it is built on: one MI355X, one process, tools/recommend_timing.py.')
    L.append('Shape: douban (3000 x 3000), hop 1, cap %d, batch 50, users 0..%d: %d candidates (%d batches); top %d per user.'
             % (a.mnph, a.users - 1, n, (n + 49) // 50, a.n))
    L.append('Every timed window is warm (%d passes of each before it: the first starts eagerly and captures its graph), ends in a'
             % a.warmup)
    L.append('device synchronise inside the clock, and the two alternate (a, b, a, b, ...).')
    L.append('')
    L.append('a  score_links over a host-built MyDynamicDataset of the same candidate list, ms per pass: ' + fmt(ms_a))
    L.append('b  recommend() end to end (enumerate + score + select + gather), ms per call:             ' + fmt(ms_b))
    L.append('')
    L.append('median a  %.3f ms  (%.3f M candidates/s)   spread max - min %.3f ms' % (med_a, n / med_a / 1e3, spread_a))
    L.append('median b  %.3f ms  (%.3f M candidates/s)   spread max - min %.3f ms' % (med_b, n / med_b / 1e3, spread_b))
    L.append('difference of the medians: %+.3f ms = %+.2f %%;  median(b) <= median(a) + spread(a):  %.3f <= %.3f  -> %s'
             % (med_b - med_a, (med_b / med_a - 1) * 100, med_b, med_a + spread_a,
                'INSIDE the spread of a' if inside else 'OUTSIDE the spread of a (see the breakdown)'))
    L.append('scores of b bit-identical to a: %s' % same)
    L.append('')
    L.append('breakdown of recommend(), ms, median of %d (each part followed by a device synchronise of its own):' % a.reps)
    for k in ('refill', 'score_candidates', 'top_n'):
        L.append('  %-18s %.3f   (%s)' % (k, statistics.median(parts[k]), fmt(parts[k])))
    L.append('  refill = 2 launches + cumsum + 2 host reads (total, error word); top_n = igmc_select_segments + the gather of link_v')
    L.append('')
    L.append('the kernels by themselves (HIP events around each launch, igmc_profile_fetch), us, median of %d (min .. max):' % a.reps)
    for name in sorted(prof):
        if name.startswith('k_candidates') or name.startswith('k_segsel'):
            us = prof[name]
            L.append('  %-20s %8.2f   (%.2f .. %.2f)' % (name, statistics.median(us), min(us), max(us)))
    L.append('  (%d candidates: the enumeration writes 8 bytes per candidate, the selection reads 4)' % n)
    text = '\n'.join(L) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
