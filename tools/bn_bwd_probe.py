"""The batch-norm layer's backward at the catalogue shape (59 047 rows, 256 features, ReLU + norm), all on the GPU: ps_bn_bwd
against torch's backward of F.batch_norm -> F.relu -> F.normalize, the peak allocation of each, and a
GraphConvLayer(256, 256) training step with grad_method "hip" against "torch".

    python tools/bn_bwd_probe.py [rounds=5] [section ...]      sections: kernel layer (default: both)

One process, HIP events.  Inside a round the methods take turns, so a ratio comes from one run; every figure is the median of the
rounds with [min .. max].  The raw output belongs under profiles/.

ps_bn_bwd has one form.  The comparison with a fused "rows" form in profiles/bn_bwd_probe.txt (run 1) was a one-off: it was made
with that kernel and a debug export that took the form, both removed when the form lost, so this tool cannot repeat it."""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommendation-engine_amd"))
import torch
import torch.nn.functional as F
from model import layers as L
from pinsage_hip import dense, sampling
from pinsage_hip import native as nv

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SECTIONS = set(sys.argv[2:]) or {"kernel", "layer"}
M, H = 59047, 256
COPY_TBS = 6.3                 # TB/s a streaming copy sustains on this memory system


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
    return f"{ms[len(ms) // 2]:9.4f} ms [{ms[0]:.4f} .. {ms[-1]:.4f}]"


def peak_of(f):
    f(); torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f(); torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


torch.manual_seed(0)
print(f"device {torch.cuda.get_device_name(0)}; rounds {ROUNDS}; M = {M}, N = {H}")

if "kernel" in SECTIONS:
    fn = nv.lib().ps_bn_bwd
    z, gy = torch.randn(M, H, device="cuda"), torch.randn(M, H, device="cuda")
    gamma, beta = torch.rand(H, device="cuda") + 0.5, torch.randn(H, device="cuda") * 0.5
    mean, var, scale = dense.batch_norm_stats(z, gamma, 1e-5, 0.1)
    gz, dg, db = torch.empty_like(z), torch.empty(H, device="cuda"), torch.empty(H, device="cuda")
    wsb = nv.lib().ps_bn_bwd_workspace_bytes(M, H)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    flags = nv.PS_RELU | nv.PS_L2NORM

    def hip():
        rc = fn(nv.ptr(z), nv.ptr(gy), M, H, nv.ptr(mean), nv.ptr(var), nv.ptr(scale), nv.ptr(beta), 1e-5, flags, nv.ptr(gz),
                nv.ptr(dg), nv.ptr(db), nv.ptr(ws), wsb, nv.stream())
        assert rc == 0, rc

    zt, gt, bt = z.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y = F.normalize(F.relu(F.batch_norm(zt, None, None, gt, bt, training=True, eps=1e-5)), p=2, dim=1)

    def torch_bwd():
        torch.autograd.grad(y, (zt, gt, bt), gy, retain_graph=True)

    def torch_fwd_bwd():
        yy = F.normalize(F.relu(F.batch_norm(zt, None, None, gt, bt, training=True, eps=1e-5)), p=2, dim=1)
        torch.autograd.grad(yy, (zt, gt, bt), gy)

    def hip_fwd_bwd():
        m, v, s = dense.batch_norm_stats(z, gamma, 1e-5, 0.1)
        dense.batch_norm_apply(z, m, s, beta, True, True)
        dense.batch_norm_bwd(z, gy, m, v, s, beta, 1e-5, True, True)

    r = rounds({"hip": hip, "torch backward": torch_bwd})
    sweep_mb = M * H * 4 / 1e6
    for k, ms in r.items():
        med = ms[len(ms) // 2]
        sweeps = 7
        note = ""
        if k.startswith("hip"):
            bound = sweeps * sweep_mb / 1e6 / COPY_TBS * 1e3
            note = f"  {sweeps} sweeps x {sweep_mb:.1f} MB = {bound * 1e3:.1f} us at {COPY_TBS} TB/s: {bound / med:.2f} of that bound"
        print(f"bn backward {M} x {H} relu+norm  {k:<15s} {fmt(ms)}{note}")
    a = gz.clone()
    hip(); torch.cuda.synchronize()
    ref = torch.autograd.grad(y, (zt, gt, bt), gy, retain_graph=True)
    print(f"   twice identical: {torch.equal(a, gz)}; max |hip - torch| gz {(gz - ref[0]).abs().max().item():.3e}, "
          f"dgamma {(dg - ref[1]).abs().max().item():.3e}, dbeta {(db - ref[2]).abs().max().item():.3e}")
    r = rounds({"hip": hip_fwd_bwd, "torch": torch_fwd_bwd})
    for k, ms in r.items():
        print(f"bn forward + backward {M} x {H} relu+norm  {k:<6s} {fmt(ms)}")
    print(f"   peak allocation, forward + backward: hip {peak_of(hip_fwd_bwd):.1f} MB, torch {peak_of(torch_fwd_bwd):.1f} MB; "
          f"backward workspace {wsb / 1e6:.2f} MB")

if "layer" in SECTIONS:
    layer = L.GraphConvLayer(H, H).cuda().train()
    xs, ns = torch.randn(M, H, device="cuda"), torch.randn(M, H, device="cuda")
    G = torch.randn(M, H, device="cuda")

    def step(method):
        def run():
            old = sampling.grad_method
            sampling.grad_method = "hip"
            layer.grad_method = method
            try:
                layer.zero_grad(set_to_none=True)
                (layer(xs, ns) * G).sum().backward()
            finally:
                sampling.grad_method = old
        return run
    fns = {"hip": step("hip"), "torch": step("torch")}
    for k, ms in rounds(fns, n=5).items():
        print(f"GraphConvLayer({H}, {H}) training step, M = {M}  {k:<6s} {fmt(ms)}")
    print("   peak allocation: " + ", ".join(f"{k} {peak_of(f):.1f} MB" for k, f in fns.items()))
