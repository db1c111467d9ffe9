"""The second level of the two-level LSH search at the catalogue shape (59 047 items, 10 000 queries, k = 10), all on the GPU:
ps_rerank_topk against the torch composition on the same inputs (E[cand] gather, bmm, topk: other tie and rounding behaviour, so
a time only), and the whole refined LSHIndex.search_device beside the unrefined one and the flat exact search (dense.dot_topk),
with the recall@10 of each against the exact result.

    python tools/rerank_probe.py [rounds=5] [section ...]      sections: kernel search (default: both)

One process, HIP events.  Inside a round the methods take turns, so a ratio comes from one run; every figure is the median of the
rounds of 10 calls with [min .. max].  The raw output belongs under profiles/ (profiles/rerank_probe.txt).  The candidate lists of
the kernel section are what the first level returns for these queries at k = R (256-bit codes), pads and all."""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommendation-engine_amd"))
import numpy as np
import torch
from pinsage_hip import dense
from utils.nearest_neighbors import LSHIndex

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SECTIONS = set(sys.argv[2:]) or {"kernel", "search"}
N, NQ, K, BITS = 59047, 10000, 10, 256


def timed(f, n):
    f(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def rounds(fns, n=10):
    """{name: sorted per-call ms of every round}; the functions take turns inside a round"""
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            out[k].append(timed(f, n))
    return {k: sorted(v) for k, v in out.items()}


def fmt(ms):
    return f"{ms[len(ms) // 2]:9.3f} ms [{ms[0]:.3f} .. {ms[-1]:.3f}]"


def items(D):
    """unit rows around 400 Gaussian centres: neighbours that a sign hash can find, as item embeddings have"""
    g = torch.Generator(device="cuda").manual_seed(D)
    centres = torch.randn(400, D, device="cuda", generator=g)
    x = centres[torch.randint(0, 400, (N,), device="cuda", generator=g)] + 0.7 * torch.randn(N, D, device="cuda", generator=g)
    return torch.nn.functional.normalize(x, dim=1).contiguous()


def recall(found, truth):
    hit = (found.unsqueeze(2) == truth.unsqueeze(1)).any(dim=2) & (found >= 0)
    return hit.sum().item() / truth.numel()


def torch_rerank(E, Q, cand, k):
    c = cand.clamp(min=0)
    sims = torch.bmm(E[c], Q.unsqueeze(2)).squeeze(2).masked_fill(cand < 0, float("-inf"))
    v, j = torch.topk(sims, k, dim=1)
    return v, torch.gather(cand, 1, j)


print(f"device {torch.cuda.get_device_name(0)}; rounds {ROUNDS}; {N} items, {NQ} queries, k = {K}, {BITS}-bit codes; "
      f"ps_rerank_max_candidates() = {dense.rerank_max_candidates()}")

for D in (128, 256):
    E = items(D)
    Q = E[:NQ].contiguous()
    plain = LSHIndex(D, BITS)
    plain.build(E)
    refined = LSHIndex(D, BITS)
    refined.refine_factor = 10
    refined.build(E)
    truth = dense.dot_topk(E, torch.arange(NQ, device="cuda"), K, exclude_self=False)[1]

    if "kernel" in SECTIONS:
        for R in (32, 64, 100, 1000):
            cand = plain.search_device(Q, R)[1].contiguous()
            r = rounds({"ps_rerank_topk": lambda: dense.rerank_topk(E, Q, cand, K), "torch gather + bmm + topk": lambda: torch_rerank(E, Q, cand, K)})
            gathered = NQ * R * D * 4
            for name, ms in r.items():
                med = ms[len(ms) // 2]
                print(f"D = {D:3d} R = {R:4d}  {name:<26s} {fmt(ms)}  {gathered / med / 1e9:7.3f} TB/s of gathered rows ({gathered / 1e6:.0f} MB)")
            ids = dense.rerank_topk(E, Q, cand, K)[1]
            print(f"   recall@{K} against the exact search: Hamming order {recall(cand[:, :K], truth):.4f}, re-ranked from R = {R} {recall(ids, truth):.4f}; "
                  f"ids equal to the torch composition's in {(ids == torch_rerank(E, Q, cand, K)[1]).all(dim=1).float().mean().item():.4f} of the rows")

    if "search" in SECTIONS:
        qidx = torch.arange(NQ, device="cuda")
        fns = {"LSH, Hamming order (k = 10)": lambda: plain.search_device(Q, K),
               "LSH + exact re-rank (R = 100)": lambda: refined.search_device(Q, K),
               "flat exact search (dot_topk)": lambda: dense.dot_topk(E, qidx, K, exclude_self=False)}
        got = {"LSH, Hamming order (k = 10)": plain.search_device(Q, K)[1], "LSH + exact re-rank (R = 100)": refined.search_device(Q, K)[1],
               "flat exact search (dot_topk)": truth}
        for name, ms in rounds(fns).items():
            print(f"D = {D:3d} search_device, {NQ} queries  {name:<30s} {fmt(ms)}  recall@{K} {recall(got[name], truth):.4f}")
    del plain, refined, E, Q
    torch.cuda.empty_cache()
