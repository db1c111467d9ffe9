"""GraphConv edge-branch aggregation at ML-25M shape, all on the GPU: the atomic forward (ps_spmm_csr) against torch index_add_,
the exact forward (ps_spmm_csr_exact), its backward for x (the same kernel over the source-grouped CSR) and for the edge values
(ps_sddmm_csr), and one GraphConv training step with each sampling.grad_method.

    python tools/spmm_probe.py [H=256] [rounds=3]

Every figure is the median over `rounds` rounds of device-event time per call; the kernels are timed in turn inside a round, so
the ratio exact : atomic comes from one run.  The torch method builds [E, H] tensors (its step peaked at 2.2 of them when
measured; 3 are budgeted), so its step is timed at the largest H of 256, 128, ... whose tensors fit the free memory, and the HIP
step at that H too."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommendation-engine_amd"))
import torch
from pinsage_hip import graph as G, sampling, synth
from model.pinsage import GraphConv

H = int(sys.argv[1]) if len(sys.argv) > 1 else 256
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
cfg = dict(synth.ML25M)
ei, ew = synth.bipartite_ratings(device="cuda", **cfg)
ew = ew.float()
V = cfg["num_users"] + cfg["num_items"]
E = ei.size(1)
x = torch.randn(V, H, device="cuda")
g = torch.randn(V, H, device="cuda")
t0 = time.time(); tc = G.TargetCSR(ei, V); torch.cuda.synchronize(); print(f"TargetCSR build {time.time()-t0:.3f}s  V={V} E={E}")
t0 = time.time(); sc, index = tc.source(); torch.cuda.synchronize(); print(f"source CSR + index build {time.time()-t0:.3f}s")
val = ew[tc.perm].contiguous()
sval = val[index].contiguous()
deg = (tc.rowptr[1:] - tc.rowptr[:-1])
S = G.nv.lib().ps_spmm_exact_slice()
print(f"slice {S}: max in-degree {int(deg.max())}, rows cut by a slice boundary <= {(E + S - 1) // S - 1}, "
      f"workspace {G.nv.lib().ps_spmm_csr_exact_workspace_bytes(E, H) / 1e6:.1f} MB")


def timed(f, n=5):
    f(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def rounds(fns, n=5):
    """{name: sorted per-call ms of every round}; the functions take turns inside a round"""
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            out[k].append(timed(f, n))
    return {k: sorted(v) for k, v in out.items()}


def show(name, ms, note=""):
    med = ms[len(ms) // 2]
    print(f"{name:<28s} {med:9.3f} ms  (min {ms[0]:.3f}, max {ms[-1]:.3f})  "
          f"gather {E*H*4/med/1e6:8.1f} GB/s logical, {E/med/1e6:.2f} Gedge/s  {note}")
    return med


r = rounds({"atomic": lambda: G.spmm_csr(tc, x, val), "exact": lambda: G.spmm_csr_exact(tc, x, val),
            "dx": lambda: G.spmm_csr_exact(sc, g, sval), "dval": lambda: G.sddmm_csr(tc, x, g)})
a = show("ps_spmm_csr", r["atomic"])
e = show("ps_spmm_csr_exact", r["exact"], f"exact : atomic = {r['exact'][len(r['exact']) // 2] / a:.3f}")
show("exact backward for x", r["dx"])
show("ps_sddmm_csr", r["dval"])
o1, o2 = G.spmm_csr(tc, x, val), G.spmm_csr_exact(tc, x, val)
print("exact against atomic, max rel diff", ((o1 - o2).abs().max() / o2.abs().max()).item(),
      " exact twice identical:", torch.equal(o2, G.spmm_csr_exact(tc, x, val)))
del o1, o2

free = torch.cuda.mem_get_info()[0]
Ht = next((h for h in (256, 128, 64, 32, 16, 8) if h <= H and 3 * E * h * 4 < 0.8 * free), None)
ms2 = timed(lambda: torch.zeros_like(x).index_add_(0, ei[1], x[ei[0]] * ew.view(-1, 1)), n=2) if 3 * E * H * 4 < 0.8 * free else None
if ms2 is not None:
    print(f"torch idx_add {ms2:8.3f} ms  ({ms2/a:.1f}x the atomic kernel)")


def step_of(h):
    torch.manual_seed(0)
    conv = GraphConv(h, h).cuda()
    xs = torch.randn(V, h, device="cuda")

    def step():
        conv.zero_grad(set_to_none=True)
        conv(xs, ei, ew).square().sum().backward()
    return step


for h in sorted({H, Ht} - {None}, reverse=True):
    step = step_of(h)
    sampling.grad_method = "hip"
    ms = rounds({"hip": step}, n=3)["hip"]
    print(f"GraphConv step, H = {h}, grad_method hip   {ms[len(ms) // 2]:9.3f} ms  (min {ms[0]:.3f}, max {ms[-1]:.3f})")
    if h == Ht:
        sampling.grad_method = "torch"
        torch.cuda.reset_peak_memory_stats()
        ms = rounds({"torch": step}, n=2)["torch"]
        print(f"GraphConv step, H = {h}, grad_method torch {ms[len(ms) // 2]:9.3f} ms  (min {ms[0]:.3f}, max {ms[-1]:.3f})  "
              f"peak {torch.cuda.max_memory_allocated() / 1e9:.1f} GB; the largest H of the list that fits {free / 1e9:.0f} GB free")
        sampling.grad_method = "hip"
    del step
    torch.cuda.empty_cache()
if Ht is None:
    print("grad_method torch: no H of the list fits the free memory")
