"""The conventions include/pinsage_hip.h opens with, held for every entry point that takes a stream (tests/helpers/abi_cases.py has
one case each, and further forms of two of them): all work is enqueued on the given stream, nothing synchronises or allocates, inputs are never written, nothing
is written outside the outputs and the workspace, the call can be captured into a hipGraph, and its results do not depend on what
the outputs or the workspace held before it.

The C ABI is called directly.  Every buffer exists before the first call; every output and the workspace is the front of its own
allocation of 0xFF bytes with a guard band behind it, the workspace exactly as large as its *_workspace_bytes function says.
Per entry point, in order:
  1. an eager call on the default stream: expected outputs bit for bit, guard bands intact, inputs unchanged;
  2. the same on a side stream;
  3. one capture of one call on the side stream (not for the two entry points documented to synchronise);
  4. replay A: re-poisoned outputs and workspace, the same three checks;
  5. replay B: the second input set copied into the same input tensors, its own expectation;
  6. replays C and D: input set B again, outputs and workspace left as the previous replay left them: the bits of replay B.
All comparisons are of bytes.  One process, one thread, single-stream graphs; nothing is retried."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import abi_cases as ac

pytestmark = pytest.mark.gpu
GUARD = 256
FILL = 0xFF


class _Buf:
    """`nbytes` bytes at the front of an allocation of their own, GUARD bytes of guard band behind them"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.view = self.raw[:self.nbytes]

    def poison(self):
        self.raw.fill_(FILL)

    def guard_intact(self):
        return bool((self.raw[self.nbytes:] == FILL).all())

    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr())

    def host(self, shape, dtype):
        return self.view.cpu().numpy().view(dtype).reshape(shape)


def _bytes(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy())


class _Harness:
    def __init__(self, c):
        from pinsage_hip import native as nv
        self.c, self.nv = c, nv
        self.fn = getattr(nv.lib(), c.name)
        self.sets = [{k: _bytes(v).cuda() for k, v in s.items()} for s in c.inputs]
        for k, (producer, out) in c.derived.items():              # inputs only the library can make: another case's output
            p = _Harness(ac.get(producer))
            for which in (0, 1):
                p.load(which)
                p.poison(ws_zero=True)
                rc = p.call()
                assert rc == 0, f"{c.name}: status {rc} from {producer}, which makes the input {k}"
                torch.cuda.synchronize()
                assert p.out[out].nbytes == self.sets[which][k].numel()
                self.sets[which][k] = p.out[out].view.clone()
        self.inp = {k: t.clone() for k, t in self.sets[0].items()}          # the tensors every call reads
        self.snap = {k: t.clone() for k, t in self.inp.items()}
        self.dtypes = dict(c.outputs)
        self.dtypes.update({k: (v.shape, v.dtype) for k, v in c.inout.items()})
        self.out = {k: _Buf(int(np.prod(shape)) * np.dtype(dt).itemsize) for k, (shape, dt) in c.outputs.items()
                    if not self._is_host_out(k)}
        self.io = {k: _Buf(v.nbytes) for k, v in c.inout.items()}
        self.io_init = {k: _bytes(v).cuda() for k, v in c.inout.items()}
        self.ws_bytes = c.workspace_bytes()
        self.ws = _Buf(self.ws_bytes) if c.ws is not None else None
        self.hosts = {k: np.ascontiguousarray(v) for k, v in c.host.items()}
        self.hout = {k: ctypes.c_int64(-1) for k in c.outputs if self._is_host_out(k)}
        self.expect = [dict(e) for e in c.expect]
        torch.cuda.synchronize()

    def _is_host_out(self, k):
        return any(isinstance(a, ac.HO) and a.name == k for a in self.c.args)

    def args(self):
        out = []
        for a in self.c.args:
            if isinstance(a, ac.I):
                out.append(ctypes.c_void_p(self.inp[a.name].data_ptr()))
            elif isinstance(a, ac.O):
                out.append(self.out[a.name].ptr())
            elif isinstance(a, ac.IO):
                out.append(self.io[a.name].ptr())
            elif isinstance(a, ac.HI):
                out.append(ctypes.c_void_p(self.hosts[a.name].ctypes.data))
            elif isinstance(a, ac.HO):
                out.append(ctypes.c_void_p(ctypes.addressof(self.hout[a.name])))
            elif a is None:
                out.append(ctypes.c_void_p(0))
            elif a == ac.WS:
                out.append(self.ws.ptr())
            elif a == ac.WSB:
                out.append(self.ws_bytes)
            elif a == ac.ST:
                out.append(self.nv.stream())
            else:
                out.append(a)
        return out

    def call(self):
        return self.fn(*self.args())

    def load(self, which):
        for k, t in self.sets[which].items():
            self.inp[k].copy_(t)
            self.snap[k].copy_(t)

    def reset_inout(self):
        for k, b in self.io.items():
            b.view.copy_(self.io_init[k])

    def poison(self, ws_zero=False):
        for b in self.out.values():
            b.poison()
        if self.ws is not None:
            self.ws.poison()
            if ws_zero:
                self.ws.view.zero_()
        for h in self.hout.values():
            h.value = -1
        self.reset_inout()

    def results(self):
        """{name: bytes} of every output and in-out buffer, unordered records sorted and cut to their count"""
        torch.cuda.synchronize()
        got = {}
        for k, b in list(self.out.items()) + list(self.io.items()):
            got[k] = b.host(*self.dtypes[k])
        for rec, cnt in self.c.unordered.items():
            n = int(got[cnt].reshape(-1)[0])
            flat = got[rec].reshape(got[rec].shape[0], -1)
            assert 0 <= n <= flat.shape[0], (self.c.name, rec, n)
            rest = flat[n:].view(np.uint8)
            assert (rest == FILL).all(), f"{self.c.name}: {rec} is written past its {n} records"
            got[rec] = ac.sort_records(flat[:n])
        for k, h in self.hout.items():
            got[k] = np.array([h.value], np.int64)
        return got

    def check(self, step, which, want=None):
        name = self.c.name
        got = self.results()
        want = self.expect[which] if want is None else want
        for k, w in want.items():
            w = ac.sort_records(w.reshape(w.shape[0], -1)) if k in self.c.unordered else w
            g = got[k]
            assert g.shape == w.shape, f"{name}, {step}: {k} has shape {g.shape}, expected {w.shape}"
            if g.tobytes() != w.tobytes():
                gb, wb = g.reshape(-1).view(np.uint8), np.ascontiguousarray(w).reshape(-1).view(np.uint8)
                bad = np.flatnonzero(gb != wb)
                e = int(bad[0]) // g.dtype.itemsize
                raise AssertionError(f"{name}, {step}: {k} differs in {len(bad)} bytes, first at element {e}: "
                                     f"got {g.reshape(-1)[e]!r}, expected {np.ascontiguousarray(w).reshape(-1)[e]!r}")
        for k, b in list(self.out.items()) + list(self.io.items()) + ([("workspace", self.ws)] if self.ws is not None else []):
            assert b.guard_intact(), f"{name}, {step}: bytes behind {k} were written"
        for k, t in self.inp.items():
            assert torch.equal(t, self.snap[k]), f"{name}, {step}: input {k} was written"
        for k, hv in self.hout.items():                           # the host's copy of a device output the call synchronised for
            dev = self.c.host_copy[k]
            assert hv.value == int(got[dev].reshape(-1)[0]), f"{name}, {step}: *{k} = {hv.value} differs from the device {dev}"
        return got

    def eager_expectations(self):
        """for outputs without an independent oracle: the eager call on the default stream with a zero-filled workspace"""
        names = self.c.eager_outputs
        if not names:
            return
        for which in (0, 1):
            self.load(which)
            self.poison(ws_zero=True)
            rc = self.call()
            assert rc == 0, f"{self.c.name}: status {rc} from the eager call that sets the expectation"
            got = self.results()
            for k in names:
                self.expect[which][k] = got[k]
        assert any(self.expect[0][k].tobytes() != self.expect[1][k].tobytes() for k in self.expect[0]), \
            f"{self.c.name}: the two input sets give the same outputs"
        self.load(0)


_faulted = []          # the entry point after which the device no longer answers: nothing more is started on it


@pytest.mark.parametrize("name", sorted(ac.CASES) + sorted(ac.VARIANTS))
def test_contract(name):
    if _faulted:
        pytest.fail(f"not run: the device reported an error during {_faulted[0]}")
    try:
        _contract(name)
    except AssertionError:
        raise
    except BaseException:
        _faulted.append(name)
        raise


def _contract(name):
    c = ac.get(name)
    h = _Harness(c)
    nv = h.nv
    main = torch.cuda.current_stream()
    assert main.cuda_stream == torch.cuda.default_stream().cuda_stream
    h.eager_expectations()

    # 1: eager, default stream
    h.poison()
    rc = h.call()
    assert rc == 0, f"{name}: status {rc} on the default stream"
    h.check("eager call on the default stream", 0)

    # 2: eager, side stream
    side = torch.cuda.Stream()
    h.poison()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        assert nv.stream().value == side.cuda_stream
        rc = h.call()
    main.wait_stream(side)
    assert rc == 0, f"{name}: status {rc} on a side stream"
    h.check("eager call on a side stream", 0)

    if c.synchronises:
        # no capture: set B and a rerun over the call's own leftovers, eagerly on the side stream
        h.load(1)
        h.poison()
        runs = []
        for step in ("input set B on a side stream", "dirty rerun on a side stream"):
            h.reset_inout()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                rc = h.call()
            main.wait_stream(side)
            assert rc == 0, f"{name}: status {rc}, {step}"
            runs.append(h.check(step, 1))
        assert all(runs[0][k].tobytes() == runs[1][k].tobytes() for k in runs[0]), f"{name}: the dirty rerun differs"
        return

    # 3: capture, once
    h.poison()
    g = torch.cuda.CUDAGraph()
    rc, st, err = None, None, None
    try:
        with torch.cuda.graph(g, stream=side):
            st = nv.stream().value
            rc = h.call()
    except RuntimeError as e:                                    # the capture was invalidated: say by whom
        err = e
    assert err is None and rc == 0, f"{name}: capture failed, status {rc}: {err}"
    assert st == side.cuda_stream

    # 4: replay A
    h.poison()
    g.replay()
    h.check("replay A", 0)

    # 5: replay B
    h.load(1)
    h.poison()
    g.replay()
    b = h.check("replay B", 1)

    # 6: replays C and D over the call's own leftovers
    for step in ("replay C", "replay D"):
        h.reset_inout()
        g.replay()
        h.check(step + " (dirty outputs and workspace)", 1, want=b)
