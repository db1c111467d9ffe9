#!/usr/bin/env python
"""Where a workgroup of the staged LSH encode spends its time: s_memtime stamps per phase (a library whose
csrc/lsh_filter.hip was compiled with -DPS_LSHF_DEBUG=2, passed as PS_HIP_LIB).

  PS_HIP_LIB=.../libpinsage_hip_dbg2.so python tools/lsh_filter_phases.py [--planes] [rows ...]      (default: 59047 10000)

--planes: the launch that also writes the sign planes of its rows (ps_lsh_encode_planes: the index build of a step); the
planes are part of the store phase.
"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "movie-recommendation-engine_amd")]
from pinsage_hip import dense                            # noqa: E402
from pinsage_hip import native as nv                     # noqa: E402
from utils.nearest_neighbors import lsh_rotation_matrix  # noqa: E402

dev = nv.require_gpu()
raw = ctypes.CDLL(nv.SO_PATH)
D, nbits = 256, 512
S = dense.stage_lsh(torch.from_numpy(lsh_rotation_matrix(D, nbits)).to(dev))
PHASES = ("x rows -> fragments", "slabs: MFMA + sign words", "flag scan", "chains", "store")
PLANES = "--planes" in sys.argv[1:]
for n in [int(v) for v in sys.argv[1:] if v != "--planes"] or [59047, 10000]:
    x = torch.nn.functional.normalize(torch.randn(n, D, device=dev), dim=1)
    for _ in range(3):
        dense.lsh_encode(x, S, planes=PLANES)
    stamps = torch.zeros(((n + 63) // 64, 16), dtype=torch.int64, device=dev)
    assert raw.ps_debug_lsh_dump(ctypes.c_void_p(stamps.data_ptr())) == 0
    dense.lsh_encode(x, S, planes=PLANES)
    torch.cuda.synchronize()
    assert raw.ps_debug_lsh_dump(ctypes.c_void_p(0)) == 0
    t = stamps[stamps[:, 0] != 0].double()
    # s_memtime counts shader clocks and is not synchronised between XCDs: only differences inside a workgroup mean something
    print(f"{n} rows{' + planes' if PLANES else ''}: {t.size(0)} workgroups, {(t[:, 5] - t[:, 0]).mean().item() / 1e3:.1f} k cycles each (mean)")
    for i, name in enumerate(PHASES):
        d = (t[:, i + 1] - t[:, i]) / 1e3
        print(f"  {name:28s} mean {d.mean().item():6.2f} k cycles   max {d.max().item():6.2f}")
    for i, name in ((6, "barriers + slab to LDS"), (7, "prefetch issue + MFMA issue"), (8, "MFMA drain + sign words")):
        print(f"    of the slabs, wave 0: {name:28s} mean {t[:, i].mean().item() / 1e3:6.2f} k cycles")
