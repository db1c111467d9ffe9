"""The MT19937 generator's hand-back: raw word 0 (stored by the chunk kernel itself), the first uniform, and the 625-word buffer
-- 624 state words, then pos -- that comes back in one copy, against np.random.RandomState."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from mt_cases import state_at as _state_at, temper as _temper  # noqa: E402  (shared with tests/test_hip_mt_stream.py)

pytestmark = pytest.mark.gpu

N = 1 << 17                               # the smallest request that takes the parallel generator


def _raw_call(rs, n, ranges=None):
    """ps_mt19937_raw_stream from rs's state, through the C ABI: (raw words, the 625-word hand-back buffer)"""
    from pinsage_hip import dense
    from pinsage_hip import native as nv
    dev = torch.device("cuda")
    _, key, pos, _, _ = rs.get_state()
    st_in = torch.from_numpy(key.astype(np.uint32).view(np.int32)).to(dev)
    back = torch.full((625,), -1, dtype=torch.int32, device=dev)
    raw = torch.full((2 * n + 1248,), -1, dtype=torch.int32, device=dev)
    polys, rpolys, wpolys = dense._jump_polys(dev), dense._radix_polys(dev), dense._window_polys(dev)
    ws, wsb = nv.workspace("ps_mt19937_workspace_bytes", dev, 0, n)
    rg = None if ranges is None else np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2))
    nv.call("ps_mt19937_raw_stream", nv.ptr(st_in), int(pos), n, nv.ptr(raw), nv.ptr(back), nv.ptr(back[624:]), nv.ptr(polys),
            polys.size(0), nv.ptr(rpolys), rpolys.size(0), nv.ptr(wpolys), wpolys.size(0), rg.ctypes.data if rg is not None else None,
            0 if rg is None else rg.shape[0], nv.ptr(ws), wsb, nv.stream())
    return raw.cpu().numpy().view(np.uint32), back.cpu().numpy().view(np.uint32)


def _check(raw, back, pos_in, uniforms_at=(0,)):
    ref = _state_at(pos_in)
    u = ref.random_sample(N)
    for i in uniforms_at:
        a, b = _temper(raw[2 * i]), _temper(raw[2 * i + 1])
        assert ((int(a) >> 5) * 67108864.0 + (int(b) >> 6)) / 9007199254740992.0 == u[i], (pos_in, i)
    _, key, pos, _, _ = ref.get_state()
    assert np.array_equal(back[:624], key.astype(np.uint32)), pos_in
    assert int(back[624]) == pos, (pos_in, int(back[624]), pos)            # the buffer's last word is pos


@pytest.mark.parametrize("pos_in", [0, 1, 623, 624])
def test_word0_state_and_pos(pos_in):
    rs = _state_at(pos_in)
    raw, back = _raw_call(rs, N)
    # raw word 0 is the untempered word the state stands on: word pos_in of the block, or the next block's first at 624
    probe = _state_at(pos_in)
    first = probe.randint(0, 2 ** 32, dtype=np.uint64)     # tempered word 0 of the stream
    assert int(_temper(raw[0])) == int(first), pos_in
    if pos_in < 624:
        assert int(raw[0]) == int(rs.get_state()[1][pos_in])
    _check(raw, back, pos_in, uniforms_at=(0, 1, 311, 312, N - 1))


def test_ranged_request():
    """a rank of a sharded job asks for two runs of uniforms, neither holding uniform 0: word 0 and the hand-back still come"""
    pos_in = 5
    runs = [(1000, 3000), (N - 4096, N - 1)]
    raw, back = _raw_call(_state_at(pos_in), N, ranges=runs)
    assert int(_temper(raw[0])) == int(_state_at(pos_in).randint(0, 2 ** 32, dtype=np.uint64))
    _check(raw, back, pos_in, uniforms_at=(1000, 2999, N - 4096, N - 2))


@pytest.mark.parametrize("pos_in", [0, 624])
@pytest.mark.parametrize("advance", [True, "defer"])
def test_python_hand_back(pos_in, advance):
    """dense.mt19937_random_sample installs the state from the one 625-word copy; the pinned buffer is reused between calls"""
    from pinsage_hip import dense
    dev = torch.device("cuda")
    saved = np.random.get_state()
    try:
        for _ in range(2):                                 # twice: the second hand-back goes through the reused buffer
            np.random.set_state(_state_at(pos_in).get_state())
            ref = _state_at(pos_in)
            u = dense.mt19937_random_sample(N, dev, advance=advance)
            if advance == "defer":
                dense.finish_rng_state()
            want = ref.random_sample(N)
            assert np.array_equal(u.cpu().numpy(), want)
            got, exp = np.random.get_state(), ref.get_state()
            assert np.array_equal(got[1], exp[1]) and got[2] == exp[2]
            assert np.random.random_sample() == ref.random_sample()
    finally:
        np.random.set_state(saved)
