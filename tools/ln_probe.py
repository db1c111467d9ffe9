"""The layer norm at the catalogue shape (59 047 rows, 256 features, one row in eight without neighbours), all on the GPU:
ps_layer_norm and ps_layer_norm_bwd (gx + dgamma + dbeta) against F.layer_norm followed by the torch.where, forward and backward,
and the peak allocation of each.

    python tools/ln_probe.py [rounds=5]

One process, HIP events.  Inside a round the methods take turns, so a ratio comes from one run; every figure is the median of the
rounds with [min .. max].  The raw output belongs under profiles/."""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommendation-engine_amd"))
import torch
import torch.nn.functional as F
from pinsage_hip import dense
from pinsage_hip import native as nv

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
M, H = 59047, 256
PEAK_TBS = 8.0                 # TB/s, the HBM roofline the byte counts are set against


def timed(f, n):
    f(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def rounds(fns, n=20):
    """{name: sorted per-call ms of every round}; the functions take turns inside a round"""
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            out[k].append(timed(f, n))
    return {k: sorted(v) for k, v in out.items()}


def fmt(ms):
    return f"{ms[len(ms) // 2]:9.4f} ms [{ms[0]:.4f} .. {ms[-1]:.4f}]"


def peak_of(f):
    f(); torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f(); torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


torch.manual_seed(0)
print(f"device {torch.cuda.get_device_name(0)}; rounds {ROUNDS}; M = {M}, N = {H}")
x, gy = torch.randn(M, H, device="cuda"), torch.randn(M, H, device="cuda")
gamma, beta = torch.rand(H, device="cuda") + 0.5, torch.randn(H, device="cuda") * 0.5
live = (torch.arange(M, device="cuda") % 8 != 0).to(torch.int32)
has = (live > 0)[:, None]
y, mean, rstd = dense.layer_norm_fwd(x, gamma, beta, 1e-5, live)
gx, dg, db = torch.empty_like(x), torch.empty(H, device="cuda"), torch.empty(H, device="cuda")
wsb = nv.lib().ps_layer_norm_bwd_workspace_bytes(M, H)
ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
fwd, bwd = nv.lib().ps_layer_norm, nv.lib().ps_layer_norm_bwd


def hip_fwd():
    rc = fwd(nv.ptr(x), M, H, nv.ptr(gamma), nv.ptr(beta), 1e-5, nv.ptr(live), nv.ptr(y), nv.ptr(mean), nv.ptr(rstd), nv.stream())
    assert rc == 0, rc


def hip_bwd():
    rc = bwd(nv.ptr(x), nv.ptr(gy), M, H, nv.ptr(mean), nv.ptr(rstd), nv.ptr(gamma), nv.ptr(live), nv.ptr(gx), nv.ptr(dg), nv.ptr(db),
             nv.ptr(ws), wsb, nv.stream())
    assert rc == 0, rc


xt, gt, bt = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()


def torch_expr():
    n = F.layer_norm(xt, (H,), gt, bt, 1e-5)
    return torch.where(has, n, torch.zeros_like(n))


def torch_fwd():
    with torch.no_grad():
        torch_expr()


yt = torch_expr()


def torch_bwd():
    torch.autograd.grad(yt, (xt, gt, bt), gy, retain_graph=True)


def torch_fwd_bwd():
    torch.autograd.grad(torch_expr(), (xt, gt, bt), gy)


def hip_fwd_bwd():
    yy, m, r = dense.layer_norm_fwd(x, gamma, beta, 1e-5, live)
    dense.layer_norm_bwd(x, gy, m, r, gamma, live)


mb = M * H * 4 / 1e6
need = {"forward": 2 * mb, "backward": 5 * mb}      # forward: x in, y out; backward: x and gy for the columns, again for the rows, gx out
for what, fns in (("forward", {"hip": hip_fwd, "torch": torch_fwd}), ("backward", {"hip": hip_bwd, "torch": torch_bwd}),
                  ("forward + backward", {"hip": hip_fwd_bwd, "torch": torch_fwd_bwd})):
    for k, ms in rounds(fns).items():
        med = ms[len(ms) // 2]
        note = ""
        if k == "hip" and what in need:
            bound = need[what] / 1e6 / PEAK_TBS * 1e3
            note = f"  {need[what]:.1f} MB = {bound * 1e3:.1f} us at {PEAK_TBS} TB/s: {bound / med:.2f} of that bound"
        print(f"layer norm {what:<18s} {M} x {H}  {k:<6s} {fmt(ms)}{note}")
a = gx.clone()
hip_fwd(); hip_bwd(); torch.cuda.synchronize()
ref = torch.autograd.grad(yt, (xt, gt, bt), gy, retain_graph=True)
print(f"   twice identical: {torch.equal(a, gx)}; max |hip - torch| y {(y - yt).abs().max().item():.3e}, gx {(gx - ref[0]).abs().max().item():.3e}, "
      f"dgamma {(dg - ref[1]).abs().max().item():.3e}, dbeta {(db - ref[2]).abs().max().item():.3e}")
print(f"   peak allocation, forward + backward: hip {peak_of(hip_fwd_bwd):.1f} MB, torch {peak_of(torch_fwd_bwd):.1f} MB; "
      f"backward workspace {wsb / 1e6:.2f} MB")
