"""What a held-out ranking evaluation costs beside the scoring pass it is built on (writes ``profiles/rank_eval_timing.txt``):

    python tools/rank_eval_timing.py [--users 100] [--reps 5] [--warmup 2] [--out profiles/rank_eval_timing.txt]

douban, hop 1, cap 100, batch 50, the first ``--users`` user ids (about 3 000 candidates each) and their test links as the
held-out set.  Every window is warm and ends in a device synchronise; the first two ALTERNATE in one process:

* ``score_candidates`` alone over the ``CandidateLinks`` that ``rank_eval`` fills (``dataset._recommend_links``);
* ``rank_eval`` end to end: refill, the same scoring pass, ``igmc_rank_segments``, ``igmc_rank_metrics``, the means;
* the two new launches by themselves, HIP events around each kernel (``igmc_profile_fetch``), at that size and at one
  segment of 1 Mi keys with 256 queries.

The expectation it confirms or refutes: the two launches cost less than the scoring pass's own run-to-run spread.
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
import torch  # noqa: E402
from igmc_amd import _lib, engine, preprocessing  # noqa: E402
from igmc_amd.models import IGMC  # noqa: E402
from igmc_amd.rank_eval import HeldOut, rank_eval  # noqa: E402
from igmc_amd.recommend import score_candidates  # noqa: E402
from igmc_amd.util_functions import MyDynamicDataset  # noqa: E402

NEW = ('k_rank_check', 'k_rank_find', 'k_rank_count', 'k_rank_metrics')


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(ms):
    return ', '.join('%.3f' % x for x in ms)


def kernel_times(lib, fn, reps):
    """us per launch of the new kernels, HIP events around each: {name: [one value per repeat]}."""
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
    return {k: v for k, v in prof.items() if k in NEW}


def kernel_lines(prof):
    out, calls = [], {'igmc_rank_segments': NEW[:3], 'igmc_rank_metrics': NEW[3:]}
    for name in NEW:
        if name in prof:
            us = prof[name]
            out.append('  %-16s %8.2f   (%.2f .. %.2f)' % (name, statistics.median(us), min(us), max(us)))
    for call, names in calls.items():
        out.append('  %-18s = %.2f us (sum of the medians of its kernels)'
                   % (call, sum(statistics.median(prof[k]) for k in names if k in prof)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=100)
    ap.add_argument('--mnph', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rank_eval_timing.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('rank_eval_timing.py measures on the GPU: no device found')
    with contextlib.redirect_stdout(sys.stderr):
        split = preprocessing.load_data_monti('douban', testing=True)
    (_, _, adj, trl, tru, trv, _, _, _, _, teu, tev, cv) = split
    train = MyDynamicDataset('data/ranktiming/train', adj, (tru, trv), trl, 1, 1.0, a.mnph, None, None, cv, seed=1)
    users = np.arange(a.users, dtype=np.int32)
    heldout = HeldOut.from_links(train, np.asarray(teu), np.asarray(tev))
    torch.manual_seed(1)
    model = IGMC(train, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True, adj_dropout=0.0,
                 seed=1).to('cuda')
    model.reset_parameters()
    model.eval()
    ks = (5, 10, 20)
    stats = {}
    run_b = lambda: rank_eval(model, train, heldout, ks=ks, users=users, stats=stats)
    run_b()                            # (fills dataset._recommend_links: the list both runs score)
    cands = train._recommend_links
    run_a = lambda: score_candidates(model, cands, 50)
    for _ in range(a.warmup):
        run_a()
        run_b()
    ms_a, ms_b = [], []
    for _ in range(a.reps):            # alternating: whatever else the host does hits both
        ms_a.append(timed(run_a)[0])
        ms_b.append(timed(run_b)[0])
    res = run_b()
    pu = res['per_user']
    # where rank_eval's time goes
    R = run_a()
    parts = {'refill': [], 'score_candidates': [], 'rank_segments': [], 'rank_metrics + means': []}
    from igmc_amd.rank_eval import reduce_metrics
    for _ in range(a.reps):
        parts['refill'].append(timed(lambda: cands.refill(pu['users']))[0])
        parts['score_candidates'].append(timed(run_a)[0])
        t, (pos, rank) = timed(lambda: engine.rank_segments(R, cands.link_v[:len(cands)], cands.offsets, pu['offsets'],
                                                            pu['items']))
        parts['rank_segments'].append(t)
        parts['rank_metrics + means'].append(timed(lambda: reduce_metrics(*engine.rank_metrics(rank, pu['offsets'], ks), ks)
                                                   .tolist())[0])
    lib = _lib.load()
    err = torch.zeros(1, dtype=torch.int32, device='cuda')

    def launches(keys, ids, seg_off, q_off, q_id):
        _, r = engine.rank_segments(keys, ids, seg_off, q_off, q_id, err=err)
        engine.rank_metrics(r, q_off, ks, err=err)
    prof_d = kernel_times(lib, lambda: launches(R, cands.link_v[:len(cands)], cands.offsets, pu['offsets'], pu['items']), a.reps)
    n_big, q_big = 1 << 20, 256
    g = torch.Generator(device='cuda').manual_seed(1)
    big_keys = torch.rand(n_big, device='cuda', generator=g)
    big_ids = torch.arange(n_big, dtype=torch.int32, device='cuda')
    big_off = torch.tensor([0, n_big], dtype=torch.int64, device='cuda')
    big_q = torch.randperm(n_big, device='cuda', generator=g)[:q_big].to(torch.int32)
    big_qoff = torch.tensor([0, q_big], dtype=torch.int64, device='cuda')
    prof_b = kernel_times(lib, lambda: launches(big_keys, big_ids, big_off, big_qoff, big_q), a.reps)
    p_big, r_big = engine.rank_segments(big_keys, big_ids, big_off, big_qoff, big_q)
    big_ok = bool((r_big.long() == (big_keys[None, :] > big_keys[big_q.long()][:, None]).sum(1) +
                   ((big_keys[None, :] == big_keys[big_q.long()][:, None]) &
                    (big_ids[None, :] < big_q[:, None])).sum(1)).all().item())
    n = stats['candidates']
    med_a, med_b = statistics.median(ms_a), statistics.median(ms_b)
    spread_a, spread_b = max(ms_a) - min(ms_a), max(ms_b) - min(ms_b)
    two = sum(statistics.median(prof_d[k]) for k in prof_d) / 1e3
    L = []
    L.append('Cost of a held-out ranking evaluation beside the scoring pass it is built on: one MI355X, one process, '
             'tools/rank_eval_timing.py.')
    L.append('Shape: douban (3000 x 3000), hop 1, cap %d, batch 50, users 0..%d: %d candidates (%d batches) in %d pass(es); %d '
             'held-out links' % (a.mnph, a.users - 1, n, (n + 49) // 50, stats['passes'], stats['queries']))
    L.append('(the test split of those users) of %d users, %d of them no candidates; cut-offs %s.'
             % (stats['users'], stats['not_candidates'], ', '.join(map(str, ks))))
    L.append('Every timed window is warm (%d passes of each before it), ends in a device synchronise inside the clock, and the'
             % (a.warmup + 1))
    L.append('two alternate (a, b, a, b, ...).')
    L.append('')
    L.append('a  score_candidates alone over the same CandidateLinks, ms per pass:            ' + fmt(ms_a))
    L.append('b  rank_eval() end to end (refill + score + rank + metrics + means), ms per call: ' + fmt(ms_b))
    L.append('')
    L.append('median a  %.3f ms  (%.3f M candidates/s)   spread max - min %.3f ms' % (med_a, n / med_a / 1e3, spread_a))
    L.append('median b  %.3f ms  (%.3f M candidates/s)   spread max - min %.3f ms' % (med_b, n / med_b / 1e3, spread_b))
    L.append('difference of the medians: %+.3f ms = %+.2f %%' % (med_b - med_a, (med_b / med_a - 1) * 100))
    L.append('')
    L.append('breakdown of rank_eval(), ms, median of %d (each part followed by a device synchronise of its own):' % a.reps)
    for k in parts:
        L.append('  %-22s %.3f   (%s)' % (k, statistics.median(parts[k]), fmt(parts[k])))
    L.append('  refill = 2 launches + cumsum + 2 host reads; rank_segments / rank_metrics here include their output allocations, the')
    L.append('  read of the error word and, for the metrics, the reduction to the means and their copy to the host')
    L.append('')
    L.append('the new kernels by themselves (HIP events around each launch, igmc_profile_fetch), us, median of %d (min .. max):'
             % a.reps)
    L.append(' at that size (%d segments, %d keys, %d queries):' % (stats['users'], n, stats['queries']))
    L += kernel_lines(prof_d)
    L.append(' one segment of %d keys, %d queries (geometry 0 = 64 workgroups; ranks equal to a torch count: %s):'
             % (n_big, q_big, big_ok))
    L += kernel_lines(prof_b)
    L.append('')
    L.append('the two new launches together, %.3f ms, against the spread of the scoring pass alone, %.3f ms: %s'
             % (two, spread_a, 'LESS than the spread' if two < spread_a else 'NOT less than the spread'))
    L.append('metrics of this run (untrained weights: the figures mean nothing, the run does): '
             + ', '.join('%s %.4f' % (k, v) for k, v in res.items() if isinstance(v, float)))
    text = '\n'.join(L) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
