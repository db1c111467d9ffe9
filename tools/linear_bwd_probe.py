"""The dense layers' backward at the catalogue shape (59 047 rows, 256 features), all on the GPU: ps_linear_wgrad against
torch.mm(g.t(), x), the candidate partition sizes, forward + backward of dense.linear against the torch expression, one training
step of each PinSage branch and of GraphConv(256, 256) at ML-25M shape with each method, and the peak allocation of both.

    python tools/linear_bwd_probe.py [rounds=5] [section ...]      sections: wgrad parts linear branches graphconv (default: all)

One process, HIP events.  Inside a round the methods take turns, so a ratio comes from one run; every figure is the median of the
rounds with [min .. max].  The raw output belongs under profiles/.  "hip-off" is sampling.grad_method = "hip" with
model.pinsage.HIP_LINEAR switched off for the branch: the code as it was before dense.linear was differentiable."""
import ctypes
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommendation-engine_amd"))
import torch
import torch.nn.functional as F
import model.pinsage as pin
from pinsage_hip import dense, sampling, synth
from pinsage_hip import native as nv

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SECTIONS = set(sys.argv[2:]) or {"wgrad", "parts", "linear", "branches", "graphconv"}
M, H = 59047, 256
PEAK_TF = 157.3


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


def peak_of(f):
    f(); torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f(); torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def with_method(method, f, **switch):
    def run():
        old, olds = sampling.grad_method, dict(pin.HIP_LINEAR)
        sampling.grad_method = method
        pin.HIP_LINEAR.update(switch)
        try:
            f()
        finally:
            sampling.grad_method = old
            pin.HIP_LINEAR.update(olds)
    return run


torch.manual_seed(0)
print(f"device {torch.cuda.get_device_name(0)}; rounds {ROUNDS}; P({M}) = {nv.lib().ps_linear_wgrad_partition(M)}")

if "wgrad" in SECTIONS:
    for K in (256, 512):
        g, x = torch.randn(M, H, device="cuda"), torch.randn(M, K, device="cuda")
        r = rounds({"hip": lambda: dense.linear_wgrad(g, x), "torch": lambda: (torch.mm(g.t(), x), g.sum(0))})
        fl = 2.0 * M * H * K
        for k, ms in r.items():
            med = ms[len(ms) // 2]
            print(f"wgrad {M} x {H} x {K}  {k:<6s} {fmt(ms)}  {fl / med / 1e9:7.1f} TFLOP/s = {fl / med / 1e9 / PEAK_TF:.3f} of the fp32 matrix peak")
        a, b = dense.linear_wgrad(g, x)
        a2, b2 = dense.linear_wgrad(g, x)
        ref = torch.mm(g.double().t(), x.double())
        print(f"   twice identical: {torch.equal(a, a2) and torch.equal(b, b2)}; max |hip - fp64| {(a.double() - ref).abs().max().item():.3e}, "
              f"max |torch - fp64| {(torch.mm(g.t(), x).double() - ref).abs().max().item():.3e}")
        print(f"   peak allocation: hip {peak_of(lambda: dense.linear_wgrad(g, x)):.1f} MB, torch {peak_of(lambda: torch.mm(g.t(), x)):.1f} MB")

if "parts" in SECTIONS:
    fn = nv.lib().ps_debug_linear_wgrad
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int64]
    for rows, K in ((M, 256), (M, 512), (12_500_000 // 16, 256)):
        g, x = torch.randn(rows, H, device="cuda"), torch.randn(rows, K, device="cuda")
        dW, db = torch.empty(H, K, device="cuda"), torch.empty(H, device="cuda")
        fns = {}
        for P in (128, 256, 512, 1024, 2048, 4096):
            parts = -(-rows // P)
            if parts > 65535:
                continue
            nb = 256 + parts * (H * K + H) * 4
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")

            def call(P=P, ws=ws, nb=nb):
                rc = fn(nv.ptr(g), rows, H, nv.ptr(x), K, nv.ptr(dW), nv.ptr(db), nv.ptr(ws), nb, nv.stream(), P)
                assert rc == 0, rc
            fns[f"P={P} ({parts} partitions, {4 * parts} workgroups, workspace {nb / 1e6:.0f} MB)"] = call
        for k, ms in rounds(fns).items():
            print(f"partition candidates {rows} x {H} x {K}  {k:<62s} {fmt(ms)}")

if "linear" in SECTIONS:
    xs, x2 = torch.randn(M, H, device="cuda"), torch.randn(M, H, device="cuda")
    W, W2, b = (torch.randn(H, H, device="cuda") / 16).requires_grad_(), (torch.randn(H, H, device="cuda") / 16).requires_grad_(), torch.randn(H, device="cuda").requires_grad_()
    G = torch.randn(M, H, device="cuda")
    for leaves, tag in (((W, W2, b), "weights only"), ((W, W2, b, xs, x2), "weights and inputs")):
        def step():
            for t in (xs, x2):
                t.requires_grad_(tag != "weights only")
            for t in (W, W2, b, xs, x2):
                t.grad = None
            dense.linear(xs, W, b, x2=x2, W2=W2, relu=True, l2norm=True).backward(G)
        r = rounds({"hip": with_method("hip", step), "torch": with_method("torch", step)})
        for k, ms in r.items():
            print(f"dense.linear fwd + bwd (relu, norm, two operand pairs; {tag})  {k:<6s} {fmt(ms)}")
        print(f"   peak allocation: hip {peak_of(with_method('hip', step)):.1f} MB, torch {peak_of(with_method('torch', step)):.1f} MB")
    xs.requires_grad_(False); x2.requires_grad_(False)

if "branches" in SECTIONS:
    model = pin.PinSage(H, H, H, 2).cuda()
    xs = torch.randn(M, H, device="cuda")
    ei = torch.randint(0, M, (2, 20 * M), device="cuda")
    ids = torch.randint(0, M, (M, 10), device="cuda", dtype=torch.int32)
    batch = sampling.NeighborBatch(ids, torch.randint(1, 5, (M, 10), device="cuda", dtype=torch.int32),
                                   torch.full((M,), 10, device="cuda", dtype=torch.int32))
    nb, wt = sampling.LazyNeighborList(batch, "ids"), sampling.LazyNeighborList(batch, "weights")
    kws = {"mlp": {}, "edge": {"edge_index": ei}, "pooled": {"sampled_neighbors": [nb, nb], "importance_weights": [wt, wt]}}
    for branch, kw in kws.items():
        def step():
            model.zero_grad(set_to_none=True)
            model(xs, **kw).square().mul(torch.arange(H, device="cuda")).sum().backward()
        fns = {"hip": with_method("hip", step, **{branch: True}), "hip-off": with_method("hip", step, **{branch: False}),
               "torch": with_method("torch", step)}
        for k, ms in rounds(fns, n=5).items():
            print(f"PinSage {branch:<6s} branch step ({M} x {H}, two layers)  {k:<8s} {fmt(ms)}")
        print("   peak allocation: " + ", ".join(f"{k} {peak_of(f):.1f} MB" for k, f in fns.items()))

if "graphconv" in SECTIONS:
    cfg = dict(synth.ML25M)
    ei, ew = synth.bipartite_ratings(device="cuda", **cfg)
    ew = ew.float()
    V = cfg["num_users"] + cfg["num_items"]
    conv = pin.GraphConv(H, H).cuda()
    xs = torch.randn(V, H, device="cuda")

    def step():
        conv.zero_grad(set_to_none=True)
        conv(xs, ei, ew).square().sum().backward()
    fns = {"hip": with_method("hip", step, edge=True), "hip-off": with_method("hip", step, edge=False)}
    for k, ms in rounds(fns, n=3).items():
        print(f"GraphConv({H}, {H}) step, V = {V}, E = {ei.size(1)}  {k:<8s} {fmt(ms)}")
    print("   peak allocation: " + ", ".join(f"{k} {peak_of(f) / 1e3:.2f} GB" for k, f in fns.items()))
