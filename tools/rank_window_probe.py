#!/usr/bin/env python3
"""The rank-window select against the only way to the same window without it, at the catalogue shape: ps_rank_window at
[lo, hi) = [2000, 5000) with max_target = the items, over rows of real PPR scores on SYN-25M (pinsage_hip.synth), against
ps_ppr_topk(k = hi) over the same rows -- one sweep of the row per rank.  Both are timed with HIP events on the score rows
alone (the push sweeps that make them are not in either time), each after one warm-up call of its own, and the window is
checked against the slice of the top-k ranking it replaces.

Usage: python tools/rank_window_probe.py [--scale 1.0] [--sources 64 1024] [--lo 2000] [--hi 5000] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "movie-recommendation-engine_amd"))
import torch                                                   # noqa: E402
from pinsage_hip import native as nv, ppr, synth               # noqa: E402
from utils.random_walk import RandomWalkSampler                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--sources", type=int, nargs="+", default=[64, 1024])
ap.add_argument("--lo", type=int, default=2000)
ap.add_argument("--hi", type=int, default=5000)
ap.add_argument("--picks", type=int, default=6)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--topk-reps", type=int, default=1, help="ps_ppr_topk(k = hi) takes seconds per call")
ap.add_argument("--json", default="")
a = ap.parse_args()
dev = torch.device("cuda")
U, M, R = [int(v * a.scale) for v in (synth.ML25M["num_users"], synth.ML25M["num_items"], synth.ML25M["num_ratings"])]
ei, ew = synth.bipartite_ratings(U, M, R, device=dev)
sampler = RandomWalkSampler(ei, ew, walk_length=2, num_walks=100, device=dev)
graph = sampler.graph
lo, hi, n = a.lo, a.hi, a.picks
print(f"device {torch.cuda.get_device_name(0)}; SYN-25M x {a.scale}: V={graph.V} E={graph.E}, {M} items; window [{lo}, {hi}), {n} picks")


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


result = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "V": graph.V, "items": M, "lo": lo, "hi": hi, "picks": n, "lines": []}
for S in a.sources:
    S = min(S, M)
    sources = (torch.arange(S, dtype=torch.int64) * (M // S)).tolist()      # items, spread over the id range
    rows = ppr.ppr_scores(graph, sources)                                   # fp64[S, V], source-major
    Vp = int(rows.size(1))
    positive = int((rows[:, :M] > 0).sum(1).min().item())
    window = torch.empty((S, hi - lo), dtype=torch.int32, device=dev)
    nwin = torch.empty(S, dtype=torch.int32, device=dev)
    picks = torch.empty((S, n), dtype=torch.int32, device=dev)
    u = torch.rand((S, n), dtype=torch.float64, device=dev)
    ids = torch.empty((S, hi), dtype=torch.int32, device=dev)
    scores = torch.empty((S, hi), dtype=torch.float64, device=dev)
    wts = torch.empty((S, hi), dtype=torch.float64, device=dev)
    nvalid = torch.empty(S, dtype=torch.int32, device=dev)

    def select():
        nv.call("ps_rank_window", nv.ptr(rows), S, Vp, Vp, M, None, lo, hi, nv.ptr(u), n, nv.ptr(window), nv.ptr(nwin), nv.ptr(picks),
                nv.stream())

    def topk():
        nv.call("ps_ppr_topk", nv.ptr(rows), S, Vp, Vp, M, hi, nv.ptr(ids), nv.ptr(scores), nv.ptr(wts), nv.ptr(nvalid), nv.stream())

    select()                                                                # one warm-up call each
    topk()
    torch.cuda.synchronize()
    t_sel = timed(select, a.reps)
    t_top = timed(topk, a.topk_reps)
    # the window is the slice of the ranking it replaces, sorted by id
    want = torch.where(torch.arange(hi, device=dev)[None, :] < nvalid[:, None], ids, torch.full_like(ids, 2 ** 31 - 1))[:, lo:]
    want = torch.sort(want, dim=1)[0]
    want[want == 2 ** 31 - 1] = -1
    same = bool(torch.equal(want, window)) and bool(torch.equal(nwin, (nvalid - lo).clamp(min=0)))
    row_mb = M * 8 / 1e6
    line = {"sources": S, "min_positive_items": positive, "rank_window_ms": t_sel, "ppr_topk_ms": t_top, "ratio": t_top / t_sel,
            "row_mb": row_mb, "rank_window_gb_per_s": 9 * S * row_mb / 1e3 / (t_sel / 1e3), "equal": same}
    result["lines"].append(line)
    print(f"S={S:5d}: ps_rank_window {t_sel:9.3f} ms ({line['rank_window_gb_per_s']:.0f} GB/s over 9 sweeps of {row_mb:.2f} MB rows), "
          f"ps_ppr_topk(k={hi}) {t_top:10.1f} ms, ratio {t_top / t_sel:.0f}x; fewest positive items in a row {positive}; "
          f"window == sorted top-k slice: {same}")
    del rows, ids, scores, wts
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(result, open(a.json, "w"), indent=1)
