#!/usr/bin/env python
"""How far the staged LSH encode's bf16 estimate is from the fp32 fmaf chain, on the benchmark's own embeddings.

Needs a library whose csrc/lsh_filter.hip was compiled with -DPS_LSHF_DEBUG=1 (it exports ps_debug_lsh_dump and writes every
estimate f to the buffer given there); pass it as PS_HIP_LIB.  The chain is ps_linear's output (the same fmaf chain, bit for
bit, as the oracle's).  Prints, per launch (index: all items, queries: the first --queries rows):
    max |f - chain| / (nx na)   against   c = 2^-12 max(1, D / 256)   (DESIGN.md section 4 asks for at most c / 4)
    the share of dots the rule flags, and whether any unflagged dot has the wrong sign.

  PS_HIP_LIB=.../libpinsage_hip_dbg.so python tools/lsh_filter_error.py [--dim 256] [--T 10] [--queries 10000]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "movie-recommendation-engine_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--T", type=int, default=10)
ap.add_argument("--queries", type=int, default=10000)
a = ap.parse_args()

from pinsage_hip import dense, synth                     # noqa: E402
from pinsage_hip import native as nv                     # noqa: E402
from pinsage_hip.graph import DeviceGraph                # noqa: E402
from pinsage_hip.shard import ShardedPinSage             # noqa: E402
from utils.random_walk import RandomWalkSampler          # noqa: E402
from utils.nearest_neighbors import lsh_rotation_matrix  # noqa: E402
from model.pinsage import PinSage                        # noqa: E402

dev = nv.require_gpu()
raw = ctypes.CDLL(nv.SO_PATH)
if not hasattr(raw, "ps_debug_lsh_dump"):
    sys.exit("PS_HIP_LIB must name a library built with -DPS_LSHF_DEBUG=1")

# the benchmark's default step (bench.py): SYN-25M, the seeded model, numpy RNG
src = synth.ML25M
U, M, R = src["num_users"], src["num_items"], src["num_ratings"]
D, nbits = a.dim, 2 * a.dim
ei, ew = synth.bipartite_ratings(U, M, R, seed=20240601, device=dev)
graph = DeviceGraph(ei, ew, device=dev)
sampler = RandomWalkSampler.from_graph(graph, walk_length=2, num_walks=100, rng="numpy", seed=42)
torch.manual_seed(2)
model = PinSage(128, 256, D, 2).to(dev).eval()
params = {k: v.detach().float().contiguous() for k, v in model.state_dict().items()}
A = torch.from_numpy(lsh_rotation_matrix(D, nbits)).to(dev)
pipe = ShardedPinSage(params, 2, sampler, M)
x = torch.randn(M, 128, generator=torch.Generator(device="cpu").manual_seed(1)).to(dev)
with torch.no_grad():
    np.random.seed(42)
    emb = pipe.embed(x, a.T).contiguous()
    pipe.ops.finish()

S = dense.stage_lsh(A)
assert isinstance(S, dense.StagedLsh)
c = 2.0 ** -12 * max(1.0, D / 256.0)
na = A.double().norm(dim=1)
for name, rows in (("index", emb), ("queries", emb[: a.queries].contiguous())):
    est = torch.full((rows.size(0), nbits), float("nan"), device=dev)
    assert raw.ps_debug_lsh_dump(ctypes.c_void_p(est.data_ptr())) == 0
    codes = dense.lsh_encode(rows, S)
    torch.cuda.synchronize()
    assert raw.ps_debug_lsh_dump(ctypes.c_void_p(0)) == 0
    chain = dense.linear(rows, A)
    assert torch.equal(codes, dense.lsh_encode(rows, A)), "staged codes differ from the fp32 path"
    nx = rows.double().norm(dim=1)
    scale = nx[:, None] * na[None, :]
    ratio = ((est.double() - chain.double()).abs() / scale).max().item()
    thr = c * (1 + 2.0 ** -10) ** 2 * scale
    trusted = est.double().abs() > thr
    wrong = int((((est >= 0) != (chain >= 0)) & trusted).sum().item())
    print(f"{name}: {rows.size(0)} x {nbits} dots, max |f - chain| / (nx na) = {ratio:.3e} = 2^{np.log2(ratio):.2f} "
          f"(c = 2^{np.log2(c):.0f}, c / 4 = {c / 4:.3e}: {'ok' if ratio <= c / 4 else 'TOO LARGE'}), "
          f"flagged {100.0 * (1.0 - trusted.double().mean().item()):.3f} %, unflagged dots of the wrong sign: {wrong}")
