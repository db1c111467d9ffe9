#!/usr/bin/env python3
"""How many ulp is the device's expf off on the arguments ps_attention_weights gives it in the aggregator tests?  The figure E of
tests/helpers/agg_cases.py::attention_bound.

The arguments are the table's own: d = fl(s - max) of every kept slot of agg_cases.GATE_CASES and agg_cases.CASES, from the exact
fp32 scores (agg_cases.attention_scores_exact).  tools/ubench/expf_ulp (built from expf_ulp.hip with the library's flags, on the
first run if it is not there) evaluates expf on them in one kernel; this script compares with numpy's fp64 exp of the same fp32
arguments -- the library function against the reference, not the kernel under test.  The error is counted in ulps of the fp32
binade of the exact value.

    python tools/expf_ulp.py [--out profiles/expf_ulp_attention.txt]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "helpers")]
import agg_cases as ac  # noqa: E402

BIN = os.path.join(ROOT, "tools", "ubench", "expf_ulp")
SRC = BIN + ".hip"


def arguments():
    """(label, fp32 arguments) per case"""
    out = []
    for gi, g in enumerate(ac.GATE_CASES):
        c = ac.gate_case(gi)
        s = ac.attention_scores_exact(c["u"], c["v"], c["w2"], c["raw_ids"], c["nvalid"], c["vec"])
        out.append((f"gate {gi} B{c['B']} N{g[1]} C{g[2]} T{g[3]}", ac.expf_arguments(s)))
    for ci, g in enumerate(ac.CASES):
        c = ac.case(ci)
        vec = 4 if g[2] % 4 == 0 and ci != ac.OFFSET_CASE else 1
        for scale in ((1.0, 8.0) if ci == ac.SCALED_CASE else (1.0,)):
            s = ac.attention_scores_exact(c["u"], c["v"], c["w2"] * np.float32(scale), c["raw_ids"], c["nvalid"], vec)
            out.append((f"case {ci} x{scale:g} B{g[0]} N{g[1]} C{g[2]} T{g[3]}", ac.expf_arguments(s)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(SRC):
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-o", BIN, SRC])
    args = arguments()
    flat = np.concatenate([x for _, x in args]).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "args.f32"), os.path.join(tmp, "expf.f32")
        flat.tofile(fin)
        subprocess.check_call([BIN, fin, fout])
        got = np.fromfile(fout, dtype=np.float32)
    assert got.shape == flat.shape
    want = np.exp(flat.astype(np.float64))
    ulp = 2.0 ** (np.floor(np.log2(want)) - 23)
    err = np.abs(got.astype(np.float64) - want) / ulp
    lines = ["tools/expf_ulp.py on MI355X: expf (hipcc -O3 -ffp-contract=off, the library's flags) against fp64 exp of the same fp32",
             "arguments d = fl(s - max) of the kept slots of agg_cases.GATE_CASES and agg_cases.CASES; error in ulps of the exact value's binade",
             f"{'case':<40}{'arguments':>10}{'min d':>12}{'max err / ulp':>16}"]
    pos = 0
    for label, x in args:
        e = err[pos:pos + x.size]
        pos += x.size
        lines.append(f"{label:<40}{x.size:>10}{(x.min() if x.size else 0.0):>12.4f}{(e.max() if x.size else 0.0):>16.4f}")
    worst = int(np.argmax(err))
    lines.append(f"all: {flat.size} arguments in [{flat.min():.4f}, {flat.max():.4f}], expf(0) == 1: {bool((got[flat == 0] == 1).all())}, "
                 f"maximum error {err.max():.4f} ulp at d = {float(flat[worst])!r} (expf gave {float(got[worst])!r})")
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if a.out:
        with open(a.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
