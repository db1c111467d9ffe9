#!/usr/bin/env python3
"""Phase times of the item co-occurrence graph (pinsage_hip.cooc, csrc/cooc_mfma.hip, csrc/cooc_sparse.hip) at SYN-25M scale
or at a synthetic --shape.

  prep    user ranks (groupby order), rows grouped by user / by (user, item), distinct entries and multiplicities (torch sorts)
  planes  ps_cooc_planes: operand planes + per-item stats
  pairs   ps_cooc_pairs: the upper-triangle contraction with the threshold / first-window epilogue (includes its sync);
          --method sparse: ps_cooc_pairs_sparse with the by-user lists and the row order it needs (no `planes` phase)
  keys    ps_cooc_keys: first common user and first positions per surviving pair
  order   torch.sort of the keys, then ps_cooc_emit writes edge_index / edge_weight

`floor_ms` is the upper triangle's products (M^2 / 2 x U) at the fp4 rate hamming_mfma.hip measured (8.4 P products/s): a
floor of the dense producer only.  `pair_updates_per_s` = the reference's dict updates (sum over users of d (d - 1) / 2) per
second of the `pairs` phase; for the sparse producer with distinct ratings each update is one LDS add and one LDS min.

usage: python tools/cooc_probe.py [--scale 1.0 | --shape U,M,R] [--method dense|sparse|auto] [--threshold 5] [--replace]
                                  [--reps 2] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "movie-recommendation-engine_amd")]

import torch  # noqa: E402

from pinsage_hip import cooc, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shape", default=None, help="U,M,R: synthetic rows of this shape instead of the scaled SYN-25M")
    ap.add_argument("--method", choices=cooc.METHODS, default="dense")
    ap.add_argument("--threshold", type=float, nargs="+", default=[5])
    ap.add_argument("--replace", action="store_true", help="the benchmark's with-replacement draw (int8 operand)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ml = synth.ML25M
    if a.shape:
        U, M, R = (int(x) for x in a.shape.split(","))
    else:
        U, M, R = (max(int(ml[k] * a.scale), 64) for k in ("num_users", "num_items", "num_ratings"))
    ei, _ = synth.bipartite_ratings(U, M, R, device="cuda", unique=not a.replace)
    n = ei.size(1) // 2
    users, items = (ei[0, :n] - M).contiguous(), ei[1, :n].contiguous()
    del ei
    d = torch.bincount(users).double()
    updates = float((d * (d - 1) / 2).sum())
    mult = torch.unique(users * M + items, return_counts=True)[1]
    out = []
    for thr in a.threshold:
        for rep in range(a.reps):
            times, last = {}, [0.0]

            def tick(name):
                torch.cuda.synchronize()
                t = time.perf_counter()
                times[name] = (t - last[0]) * 1e3
                last[0] = t

            torch.cuda.synchronize()
            last[0] = t0 = time.perf_counter()
            e_i, e_w = cooc.item_cooccurrence_graph(users, items, M, threshold=thr, device="cuda", timer=tick, method=a.method)
            torch.cuda.synchronize()
            total = (time.perf_counter() - t0) * 1e3
            P = e_w.numel() // 2
            del e_i, e_w
            floor = M * M / 2.0 * U / 8.4e15 * 1e3
            r = dict(method=a.method, planes_phase="planes" in times, users=U, items=M, rows=n, unique=not a.replace,
                     max_mult=int(mult.max()), threshold=thr, rep=rep, pairs=P, ref_dict_updates=updates, total_ms=round(total, 2),
                     pair_updates_per_s=round(updates / (times["pairs"] * 1e-3), 1), floor_ms=round(floor, 2),
                     **{k + "_ms": round(v, 2) for k, v in times.items()})
            if "planes" in times:
                r["pairs_fraction_of_floor"] = round(floor / times["pairs"], 4)
            print(json.dumps(r), flush=True)
            out.append(r)
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
