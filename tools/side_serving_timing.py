"""Wall time of score_links over a side-feature dataset of 20 000 links (rows gathered by link position, k_side_gather) against
score_candidates over CandidateLinks.from_pairs of the same links (rows gathered by node id, k_side_gather_nodes), alternating in
one process on the GPU: ``python tools/side_serving_timing.py`` (profiles/side_serving_timing.txt holds a run)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from igmc_amd import preprocessing                                   # noqa: E402
from igmc_amd.models import IGMC                                     # noqa: E402
from igmc_amd.recommend import CandidateLinks, score_candidates      # noqa: E402
from igmc_amd.train_eval import score_links                          # noqa: E402
from igmc_amd.util_functions import MyDynamicDataset                 # noqa: E402

N, B, CAP, REPS = 20000, 50, 100, 7
(_, _, adj, trl, tru, trv, _, _, _, _, _, _, cv) = preprocessing.load_data_monti('flixster', testing=True)
rng = np.random.default_rng(0)
uf = rng.standard_normal((adj.shape[0], 12)).astype(np.float32)
vf = rng.standard_normal((adj.shape[1], 20)).astype(np.float32)
ds = MyDynamicDataset('data/t/side_timing', adj, (tru[:N], trv[:N]), trl[:N], 1, 1.0, CAP, uf, vf, cv, seed=2)
torch.manual_seed(4)
model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True, adj_dropout=0.2,
             side_features=True, n_side_features=32, seed=3).to('cuda')
model.reset_parameters()
model.eval()
pairs = CandidateLinks.from_pairs(ds, ds.link_u, ds.link_v)


def by_position():
    return score_links(model, ds, B)[0]


def by_node():
    return score_candidates(model, pairs, B)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


a, b = by_position(), by_node()                                     # warm-up: both capture their scoring graph here
same = bool(torch.equal(a, b))
ta, tb = [], []
for _ in range(REPS):                                               # alternating, same process
    ta.append(timed(by_position)[0])
    tb.append(timed(by_node)[0])
lines = ['flixster, %d links, batch %d, max_nodes_per_hop %d, 12 + 20 side-feature columns; %d alternating repetitions after one warm-up pass each' % (N, B, CAP, REPS),
         'scores bit-equal: %s' % same,
         'score_links(dataset)             [k_side_gather, by link position]: ms per pass %s  median %.2f' % (' '.join('%.2f' % (1e3 * t) for t in ta), 1e3 * float(np.median(ta))),
         'score_candidates(from_pairs)     [k_side_gather_nodes, by node id]: ms per pass %s  median %.2f' % (' '.join('%.2f' % (1e3 * t) for t in tb), 1e3 * float(np.median(tb)))]
print('\n'.join(lines))
