#!/usr/bin/env python3
"""Personalized-PageRank neighbourhoods on SYN-25M (pinsage_hip.synth): what RandomWalkSampler.ppr_batch costs for `--sources`
item sources, per number of sweeps, with and without row skipping (PS_PPR_NO_SKIP), next to the bytes the sweeps have to move
(in-edges read x 512 B per 64-source slab), and what the "host" method costs per source.

  device   median of `--reps` calls timed with HIP events after a warm-up call, for num_iterations = 1..--sweeps; the cost of
           sweep k is the difference of two neighbouring lines
  rows     in-edge rows read per sweep with skipping, counted from the scores: a node pushed in sweep k exactly when its score
           rose in sweep k, and an in-edge u -> v is read in sweep k when u's slab pushed in sweep k (u < v) or k - 1 (u > v)
  host     ppr_method = "host" on `--host-sources` of the same sources for 1 and `--host-sweeps` sweeps (a host clock; it is
           python), extrapolated linearly to --sweeps: from the second sweep on the frontier is most of the graph
Usage: python tools/ppr_probe.py [--scale 1.0] [--sources 1024] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "movie-recommendation-engine_amd"))
import torch                                                   # noqa: E402
from pinsage_hip import ppr, synth                             # noqa: E402
from utils.random_walk import RandomWalkSampler                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--sources", type=int, default=1024)
ap.add_argument("--sweeps", type=int, default=10)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-sources", type=int, default=2)
ap.add_argument("--host-sweeps", type=int, default=2)
ap.add_argument("--json", default="")
a = ap.parse_args()
dev = torch.device("cuda")
U, M, R = [int(v * a.scale) for v in (synth.ML25M["num_users"], synth.ML25M["num_items"], synth.ML25M["num_ratings"])]
ei, ew = synth.bipartite_ratings(U, M, R, device=dev)
sampler = RandomWalkSampler(ei, ew, walk_length=2, num_walks=100, device=dev)
graph = sampler.graph
t0 = time.time()
pg = ppr.ppr_graph(graph)
torch.cuda.synchronize()
build_s = time.time() - t0
S = min(a.sources, M)
sources = (torch.arange(S, dtype=torch.int64) * (M // S)).tolist()          # items, spread over the id range
nslab = -(-S // 64)
E_in = int(pg.in_src.numel())
max_in = int((pg.in_rowptr[1:] - pg.in_rowptr[:-1]).max().item())          # the longest row: one wave per slab walks it alone
print(f"SYN-25M x {a.scale}: V={graph.V} E={graph.E} in-edges={E_in} (longest row {max_in}) levels={pg.n_levels}  "
      f"PPRGraph build {build_s:.2f} s; {S} item sources = {nslab} slabs")


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts), min(ts)


def rows_read():
    """in-edge rows read by sweep k = 0..sweeps-1 with skipping, summed over the slabs"""
    v_of = torch.repeat_interleave(torch.arange(graph.V, device=dev), pg.in_rowptr[1:] - pg.in_rowptr[:-1])
    u_of = pg.in_src.long()
    upper = u_of > v_of
    out, prev_scores = [], None
    act_prev = torch.zeros((graph.V, nslab), dtype=torch.bool, device=dev)
    for k in range(a.sweeps):
        scores = ppr.ppr_scores(graph, sources, sweeps=k + 1)                # [S, V]
        base = prev_scores if prev_scores is not None else torch.zeros_like(scores)
        if prev_scores is None:
            base[torch.arange(S, device=dev), torch.tensor(sources, device=dev)] = 1.0
        rose = (scores != base).t()                                          # [V, S]
        pad = torch.zeros((graph.V, nslab * 64 - S), dtype=torch.bool, device=dev)
        act = torch.cat([rose, pad], 1).view(graph.V, nslab, 64).any(dim=2)
        n = 0
        for sl in range(nslab):
            n += int((torch.where(upper, act_prev[u_of, sl], act[u_of, sl])).sum().item())
        out.append(n)
        act_prev, prev_scores = act, scores
        del base, rose
    return out


result = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "V": graph.V, "E": graph.E, "in_edges": E_in, "max_in_degree": max_in,
          "levels": pg.n_levels, "sources": S, "k": a.k, "reps": a.reps, "build_s": build_s, "lines": []}
skip = ppr.ppr_topk(graph, sources, a.k, sweeps=a.sweeps)
noskip = ppr.ppr_topk(graph, sources, a.k, sweeps=a.sweeps, skip_rows=False)
assert torch.equal(skip.ids, noskip.ids) and torch.equal(skip.wts, noskip.wts)
touched = rows_read()
NOSKIP_AT = {1, 2, 3, a.sweeps}                               # the no-skip sweeps all cost the same: a few lines are enough
print(f"{'sweeps':>6s} | {'skip ms':>9s} {'no-skip ms':>10s} | {'rows read (last sweep)':>22s} {'GB':>8s} {'of all':>7s}")
for k in range(1, a.sweeps + 1):
    med, best = timed(lambda: sampler.ppr_batch(sources, a.k, num_iterations=k))
    med_n, best_n = timed(lambda: ppr.ppr_topk(graph, sources, a.k, sweeps=k, skip_rows=False)) if k in NOSKIP_AT else (None, None)
    gb = touched[k - 1] * 512 / 1e9
    result["lines"].append({"sweeps": k, "skip_ms_median": med, "skip_ms_min": best, "noskip_ms_median": med_n,
                            "noskip_ms_min": best_n, "rows_read_last_sweep": touched[k - 1], "gb_last_sweep": gb,
                            "gb_last_sweep_noskip": E_in * nslab * 512 / 1e9})
    print(f"{k:6d} | {med:9.2f} {'-' if med_n is None else format(med_n, '.2f'):>10s} | {touched[k - 1]:22d} {gb:8.2f} {touched[k - 1] / (E_in * nslab):7.3f}")
push_only = timed(lambda: ppr.ppr_scores(graph, sources, sweeps=a.sweeps))[0]
result["push_and_transpose_ms"] = push_only
print(f"push sweeps + transpose alone ({a.sweeps} sweeps): {push_only:.2f} ms")

if a.host_sources > 0:
    hs = sources[:: max(1, S // a.host_sources)][: a.host_sources]
    sampler.ppr_method = "host"
    sampler._ppr_host_csr()
    times = {}
    host = {}
    for sw in (1, a.host_sweeps):
        t0 = time.time()
        host = {}
        for s_ in hs:                                             # one source per call: a line of output per source
            host.update(sampler.compute_ppr_matrix([s_], num_iterations=sw))
            print(f"  host: source {s_}, {sw} sweep(s): {time.time() - t0:.1f} s so far", flush=True)
        times[sw] = (time.time() - t0) / len(hs)
    sampler.ppr_method = "device"
    same = list(sampler.compute_ppr_matrix(hs, num_iterations=a.host_sweeps).items()) == list(host.items())
    per_sweep = (times[a.host_sweeps] - times[1]) / max(1, a.host_sweeps - 1)
    extrapolated = times[1] + per_sweep * (a.sweeps - 1)
    result["host"] = {"sources": hs, "s_per_source": times, "s_per_full_sweep": per_sweep, "s_per_source_extrapolated": extrapolated,
                      "equals_device": same}
    print(f"host method, per source: {times[1]:.2f} s for 1 sweep, {times[a.host_sweeps]:.2f} s for {a.host_sweeps}; "
          f"extrapolated to {a.sweeps} sweeps: {extrapolated:.1f} s per source; equal to the device result: {same}")
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(result, open(a.json, "w"), indent=1)
