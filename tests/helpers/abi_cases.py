"""One case per stream-taking entry point of include/pinsage_hip.h, for the contract matrix of tests/test_hip_abi_contract.py:
all work on the given stream, nothing allocated or synchronised, inputs never written, nothing written outside the outputs and
the workspace, hipGraph-capturable, and results that do not depend on what the workspace or the outputs held before the call.

CASES maps an entry point's name to a builder; a builder returns a Case:

  args      the C argument list in the header's order.  I(name) an input, O(name) an output, IO(name) a documented in-out
            buffer, HI(name) a HOST input array, HO(name) a HOST int64[1] output, WS / WSB the workspace and its size, ST the
            stream, None a NULL pointer, anything else a scalar passed as it is;
  inputs    two input sets {name: numpy array} of the same shapes and dtypes (A and B), which differ;
  outputs   {name: (shape, dtype)};
  inout     {name: numpy array}: the value every in-out buffer is reset to before a call (in-out names appear in `expect`);
  host      {name: numpy array}: host arrays (level pointers of ps_ppr_push);
  ws        (name of the *_workspace_bytes function, its arguments) or None;
  expect    two dicts {name: numpy array}, the expected outputs of the two input sets from the family's numpy restatement or the C
            oracle.  An output WITHOUT an entry has no independent oracle: its expectation is the eager call on the default
            stream with a zero-filled workspace (Case.eager_outputs lists them);
  unordered {records output: count output}: outputs documented as unordered -- the first `count` records are compared after
            sorting, the rest of the buffer must be untouched;
  derived   {input: (case, output)}: an input no host code can make (a staged image, sign planes) -- the GPU test fills it with
            that output of the named case, run on the same input set; the builder's array is a placeholder of the right size;
  host_copy {host output: device output}: every HO output is the host's copy of that device output (h_count of count);
  synchronises  the entry point is a documented exception (it synchronises its stream and reports through h_count): it is
            not captured.

Entries with an output that has no independent oracle (expectation of that output = the eager call, see above; every other
output of theirs is held to an oracle; tests/test_abi_cases.py pins this list, so that it cannot grow unnoticed):
  ps_attention_weights       attn    the softmax goes through expf: the project has a bound for it, no bits
  ps_gcn_layer(_ordered)     y       the row norm behind the GEMM: a bound, no bits
  ps_lsh_stage               staged  the bf16 image the filter kernel reads, defined by that kernel
  ps_lsh_expand              planes  the fp4 sign planes in MFMA operand order, defined by the kernels that read them
  ps_lsh_encode_planes       planes  (its codes are the C oracle's)
  ps_hardest_negative        best    the packed (similarity, index) word (sim / idx are the C oracle's)
  ps_cooc_planes             planes  the fp4 / int8 operand planes (item_stats / max_seen are restated from the header)
Written here from the header's own sentences, for want of a helper: ps_permute_k's column order, ps_cooc_planes' three sums
per item, and the LAYOUT of ps_ppr_push's inputs (ppr_cases.in_edges / levels / shares give the edges, levels and shares; the
header's summation order -- sources u > v ascending, then u < v, self-loops left out -- and the flattening into in_rowptr /
in_src / in_share / level_nodes are applied here; the GPU tests of the family take these arrays from the package's PPRGraph,
which is built on the device).  The expected PPR scores are ppr_cases.reference_scores, which knows none of that layout.
ps_rank_count counts, over the C oracle's similarities, what the header defines.  The grouped arrays of the co-occurrence
cases are the package's own host-side preparation (cooc._Prep on CPU tensors); everything expected is cooc_defs'.
VARIANTS holds further forms of entry points that have a case ("<entry point>:<form>"): the serial MT19937 generator, and
ps_lsh_expand over the queries (the planes ps_hamming_topk_mfma is given).

Every builder asserts the shape conditions that make its case worth running (the workspace path and every launch reached, no
empty launch); tests/test_abi_cases.py runs the builders on a machine without a GPU."""
import ctypes
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "movie-recommendation-engine_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


class _Ref:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return f"{type(self).__name__}({self.name!r})"


class I(_Ref):      # noqa: E742
    pass


class O(_Ref):      # noqa: E742
    pass


class IO(_Ref):
    pass


class HI(_Ref):
    pass


class HO(_Ref):
    pass


WS, WSB, ST = "<workspace>", "<workspace bytes>", "<stream>"


class Case:
    def __init__(self, name, args, inputs, outputs, expect, inout=None, host=None, ws=None, unordered=None, synchronises=False,
                 derived=None, host_copy=None):
        self.name, self.args, self.inputs, self.outputs = name, list(args), inputs, dict(outputs)
        self.derived, self.host_copy = dict(derived or {}), dict(host_copy or {})
        self.expect, self.inout, self.host, self.ws = expect, dict(inout or {}), dict(host or {}), ws
        self.unordered, self.synchronises = dict(unordered or {}), synchronises
        self._check()

    @property
    def eager_outputs(self):
        return sorted(set(self.outputs) - set(self.expect[0]) - {h.name for h in self.args if isinstance(h, HO)})

    def workspace_bytes(self):
        if self.ws is None:
            return 0
        return int(getattr(lib(), self.ws[0])(*self.ws[1]))

    def _check(self):
        from pinsage_hip import native
        a, b = self.inputs
        proto = native.PROTOTYPES[self.name].partition(" ")[2]
        assert len(self.args) == len(proto), f"{self.name}: {len(self.args)} arguments, the header declares {len(proto)}"
        for arg, code in zip(self.args, proto):
            if isinstance(arg, _Ref) or arg is None or arg in (WS, ST):
                assert code == "p", (self.name, arg, code)
            elif arg == WSB:
                assert code == "z", (self.name, arg, code)
            else:
                assert code != "p" and (isinstance(arg, float) if code == "f" else isinstance(arg, int)), (self.name, arg, code)
        assert self.args[-1] == ST and self.args.count(ST) == 1
        assert (WS in self.args) == (WSB in self.args) == (self.ws is not None), self.name
        if self.ws is not None:
            assert self.workspace_bytes() > 0, f"{self.name}: the case does not reach the workspace"
        refs = [x for x in self.args if isinstance(x, _Ref)]
        assert {x.name for x in refs if isinstance(x, I)} == set(a) == set(b), self.name
        assert {x.name for x in refs if isinstance(x, (O, HO))} == set(self.outputs), self.name
        assert {x.name for x in refs if isinstance(x, IO)} == set(self.inout), self.name
        assert {x.name for x in refs if isinstance(x, HI)} == set(self.host), self.name
        for k in a:
            assert isinstance(a[k], np.ndarray) and a[k].size > 0 and a[k].flags.c_contiguous, (self.name, k)
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (self.name, k)
        assert any(a[k].tobytes() != b[k].tobytes() for k in a), f"{self.name}: the two input sets are equal"
        for k, (shape, dtype) in self.outputs.items():
            assert int(np.prod(shape)) > 0, (self.name, k)
        ea, eb = self.expect
        assert set(ea) == set(eb) and set(ea) <= set(self.outputs) | set(self.inout), self.name
        for k in ea:
            shape, dtype = self.outputs[k] if k in self.outputs else (self.inout[k].shape, self.inout[k].dtype)
            if k not in self.unordered:
                for e in (ea[k], eb[k]):
                    assert e.shape == tuple(shape) and e.dtype == np.dtype(dtype), (self.name, k, e.shape, e.dtype, shape, dtype)
        if ea:
            assert any(ea[k].tobytes() != eb[k].tobytes() for k in ea), f"{self.name}: the two expectations are equal"
        for rec, cnt in self.unordered.items():
            assert rec in self.outputs and cnt in self.outputs
        assert set(self.host_copy) == {x.name for x in refs if isinstance(x, HO)}, self.name
        assert all(dev in self.outputs and dev not in self.host_copy for dev in self.host_copy.values()), self.name
        for k, (producer, out) in self.derived.items():
            shape, dtype = get(producer).outputs[out]
            assert a[k].nbytes == int(np.prod(shape)) * np.dtype(dtype).itemsize, (self.name, k)


def get(name):
    """the case of an entry point, or of one of the further forms in VARIANTS"""
    return (CASES[name] if name in CASES else VARIANTS[name])()


def lib():
    from pinsage_hip import native
    if not native.have_lib():
        import __graft_entry__ as ge
        ge.build()
    return native.lib()


def sort_records(a):
    """rows of a 2-d integer array in lexicographic order"""
    a = np.ascontiguousarray(a)
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def _c(a, dtype=None):
    return np.ascontiguousarray(a, dtype=dtype)


def _alpha_bits(alpha):
    return int(np.float64(alpha).view(np.uint64))


CASES = {}


def case(fn):
    name = fn.__name__.lstrip("_")
    CASES[name] = functools.lru_cache(maxsize=None)(lambda: fn(name))
    return fn


# ---- the sampler's graph (csrc/csr_build.hip, walk_sample.hip): C oracle for the CSR / CDF / walks, graph_defs for what is derived ----
# rows of 32 and 33 edges: both CDF kernels; more than 1024 edges in all: the sort of ps_csr_build beyond its one-block form
_DEG = (32, 33, 0, 1, 2, 7, 8, 9, 40, 100, 5, 16, 17, 3, 64, 65) + (4,) * 24 + (30,) * 22
_V, _E = len(_DEG), sum(_DEG)
_SINK = 2                                                                          # the one node without out-edges
_W, _L, _T = 20, 2, 8


@functools.lru_cache(maxsize=None)
def _graph(seed, reach_sink=False):
    """edge list (src, dst int64[E], w float32[E]) with the out-degrees _DEG in shuffled edge order, and its host CSR / CDF"""
    import torch
    from oracle import c_oracle as co
    from helpers import graph_defs as gd
    rs = np.random.RandomState(seed)
    src = np.repeat(np.arange(_V), _DEG)[rs.permutation(_E)].astype(np.int64)
    targets = np.arange(_V) if reach_sink else np.delete(np.arange(_V), _SINK)
    dst = targets[rs.randint(0, len(targets), _E)].astype(np.int64)
    if reach_sink:
        dst[0] = _SINK
    w = (rs.randint(1, 11, _E) / 2).astype(np.float32)
    cg = co.Graph(np.stack([src, dst]), w, num_nodes=_V)
    assert _E % 8 != 0 and _E > 256 and cg.V == _V and np.array_equal(np.diff(cg.rowptr), _DEG)
    t = {k: torch.from_numpy(getattr(cg, k)) for k in ("rowptr", "col", "cdf")}
    guide = gd.expected_guide(t["rowptr"], t["cdf"])
    g = dict(src=src, dst=dst, w=w, cg=cg, rowptr=cg.rowptr, col=cg.col, wsorted=cg.w, cdf=cg.cdf, guide=_c(guide.numpy()),
             nodeinfo=_c(np.stack([cg.rowptr[:-1], np.diff(cg.rowptr)], axis=1).reshape(-1), np.uint32),
             packed=_c(gd.expected_packed(t["col"], t["cdf"], guide).numpy().reshape(-1)),
             buckets=_c(gd.expected_full_buckets(t["rowptr"], t["col"], t["cdf"], guide).numpy().reshape(-1)),
             half=_c(gd.expected_half_buckets(t["rowptr"], t["col"], t["cdf"], guide).numpy().reshape(-1)))
    g["dest_info"] = _c(g["nodeinfo"].reshape(_V, 2)[cg.col].reshape(-1))
    return g


def _pick(g, *names):
    return {k: g[k] for k in names}


def _graph_case(name, args, ins, outs, **kw):
    ga, gb = _graph(11, True), _graph(12, False)
    return Case(name, args, (_pick(ga, *ins), _pick(gb, *ins)), {k: (ga[k].shape, ga[k].dtype) for k in outs},
                (_pick(ga, *outs), _pick(gb, *outs)), **kw)


@case
def _ps_csr_build(name):
    c = _graph_case(name, [I("src"), I("dst"), I("w"), _E, _V, O("rowptr"), O("col"), O("wsorted"), WS, WSB, ST],
                    ("src", "dst", "w"), ("rowptr", "col", "wsorted"), ws=("ps_csr_build_workspace_bytes", (_E, _V)))
    # Up to 1024 pairs rocprim sorts in one block: one launch, 256 bytes of nominal temporary storage.  Beyond that ps_csr_build's
    # configuration takes the multi-launch merge sort at every size (csrc/csr_build.hip: CsrSortConfig), which sorts through
    # temporary storage.  The size function (4 key / value arrays + the sort's storage + 256) says which form a case gets: the
    # one-block figure at E = 1024, another one here -- more with a device, 0 without (rocprim sizes that path per architecture).
    import torch
    seg = -(-_E * 4 // 256) * 256
    one_block = int(lib().ps_csr_build_workspace_bytes(1024, _V)) - 4 * 4096 - 256
    temp = c.workspace_bytes() - 4 * seg - 256
    assert _E > 1024 and one_block == 256 and temp != one_block
    assert temp > one_block if torch.cuda.is_available() else temp == 0
    return c


@case
def _ps_cdf_build(name):
    assert 32 in _DEG and 33 in _DEG
    return _graph_case(name, [I("rowptr"), I("wsorted"), _V, O("cdf"), ST], ("rowptr", "wsorted"), ("cdf",))


@case
def _ps_guide_build(name):
    return _graph_case(name, [I("rowptr"), I("cdf"), _V, O("nodeinfo"), O("guide"), ST], ("rowptr", "cdf"), ("nodeinfo", "guide"))


@case
def _ps_pack_edges(name):
    return _graph_case(name, [I("col"), I("cdf"), I("guide"), _E, O("packed"), ST], ("col", "cdf", "guide"), ("packed",))


@case
def _ps_bucket_build(name):
    return _graph_case(name, [I("rowptr"), I("col"), I("cdf"), I("guide"), _V, _E, O("buckets"), ST],
                       ("rowptr", "col", "cdf", "guide"), ("buckets",))


@case
def _ps_bucket_build_half(name):
    return _graph_case(name, [I("rowptr"), I("col"), I("cdf"), I("guide"), _V, _E, O("half"), ST],
                       ("rowptr", "col", "cdf", "guide"), ("half",))


@case
def _ps_dest_info_build(name):
    return _graph_case(name, [I("col"), I("nodeinfo"), _E, _V, O("dest_info"), ST], ("col", "nodeinfo"), ("dest_info",))


@case
def _ps_graph_stats(name):
    ga, gb = _graph(11, True), _graph(12, False)
    exp = tuple({"flags": np.array([s, max(_DEG)], np.int64)} for s in (1, 0))
    return Case(name, [I("rowptr"), I("col"), _E, _V, O("flags"), ST], (_pick(ga, "rowptr", "col"), _pick(gb, "rowptr", "col")),
                {"flags": ((2,), np.int64)}, exp)


def _starts(seed):
    rs = np.random.RandomState(seed)
    s = rs.permutation(_V).astype(np.int64)
    assert _SINK in s
    return s


@case
def _ps_uniform_offsets(name):
    ins, exp = [], []
    for seed in (13, 14):
        g, s = _graph(seed), _starts(seed)
        off, total = g["cg"].uniform_offsets(s, _W, _L)
        ins.append({"rowptr": g["rowptr"], "starts": s})
        exp.append({"uoff": off, "total": np.array([total], np.int64)})
    ins[1]["starts"] = _c(np.roll(ins[0]["starts"], 7))           # the same graph shape, the isolated node elsewhere
    exp[1]["uoff"] = _graph(14)["cg"].uniform_offsets(ins[1]["starts"], _W, _L)[0]
    return Case(name, [I("rowptr"), _V, I("starts"), _V, _W, _L, O("uoff"), O("total"), ST], tuple(ins),
                {"uoff": ((_V,), np.int64), "total": ((1,), np.int64)}, tuple(exp))


_WALK_IN = ("rowptr", "col", "cdf", "nodeinfo", "guide", "packed", "half", "dest_info")


def _walk_out(layers=None):
    lead = () if layers is None else (layers,)
    return {"ids": (lead + (_V, _T), np.int32), "counts": (lead + (_V, _T), np.int32), "nvalid": (lead + (_V,), np.int32)}


@case
def _ps_walk_sample(name):
    """the numpy stream, every accelerator given: node records, guide, packed blocks, half bucket records, destination records"""
    from oracle import c_oracle as co
    from pinsage_hip import native as nv
    ins, exp = [], []
    for seed in (13, 14):
        g, s = _graph(seed), _starts(seed)
        uoff, n = g["cg"].uniform_offsets(s, _W, _L)
        u = np.random.RandomState(seed).random_sample(n)
        ids, counts, nvalid = co.walk_sample(g["cg"], s, _T, _L, _W, uniforms=u, uoff=uoff)[:3]
        assert (nvalid == _T).any() and (nvalid == 0).any()
        ins.append(dict(_pick(g, *_WALK_IN), starts=s, uniforms=u, uoff=uoff))
        exp.append({"ids": ids.astype(np.int32), "counts": counts, "nvalid": nvalid})
    return Case(name, [I("rowptr"), I("col"), I("cdf"), _V, I("starts"), _V, _W, _L, _T, nv.PS_RNG_STREAM | nv.PS_WALK_HALF_BUCKETS,
                       I("uniforms"), I("uoff"), 0, 0, I("nodeinfo"), I("guide"), I("packed"), I("half"), I("dest_info"),
                       O("ids"), O("counts"), O("nvalid"), ST], tuple(ins), _walk_out(), tuple(exp))


@case
def _ps_walk_sample_layers(name):
    """Philox, two layers in one launch"""
    from oracle import c_oracle as co
    from pinsage_hip import native as nv
    layers, seed0, call = 2, 0x1234567890, 5
    ins, exp = [], []
    for seed in (13, 14):
        g, s = _graph(seed), _starts(seed)
        r = [co.walk_sample(g["cg"], s, _T, _L, _W, philox=(seed0, call + l))[:3] for l in range(layers)]
        ins.append(dict(_pick(g, *_WALK_IN), starts=s))
        exp.append({"ids": np.stack([x[0] for x in r]).astype(np.int32), "counts": np.stack([x[1] for x in r]),
                    "nvalid": np.stack([x[2] for x in r])})
    return Case(name, [I("rowptr"), I("col"), I("cdf"), _V, I("starts"), _V, _W, _L, _T, nv.PS_RNG_PHILOX | nv.PS_WALK_HALF_BUCKETS,
                       None, None, 0, seed0, call, I("nodeinfo"), I("guide"), I("packed"), I("half"), I("dest_info"), layers,
                       O("ids"), O("counts"), O("nvalid"), ST], tuple(ins), _walk_out(layers), tuple(exp))


@case
def _ps_walk_paths(name):
    from oracle import c_oracle as co
    from pinsage_hip import native as nv
    L, ins, exp = 3, [], []
    for seed in (13, 14):
        g = _graph(seed)
        s = np.repeat(_starts(seed), 2)
        B = len(s)
        u = np.random.RandomState(seed + 100).random_sample(B * L)
        uoff = np.arange(B, dtype=np.int64) * L
        paths = np.full((B, L), -1, np.int32)
        for i in range(B):
            p = co.single_walk(g["cg"], s[i], L, u, pos=int(uoff[i]))[0][1:]
            paths[i, :len(p)] = p
        assert (paths[:, -1] >= 0).any() and (paths[:, 0] < 0).any()
        ins.append(dict(_pick(g, "rowptr", "col", "cdf", "nodeinfo", "guide"), starts=s, uniforms=u, uoff=uoff))
        exp.append({"paths": paths})
    B = 2 * _V
    return Case(name, [I("rowptr"), I("col"), I("cdf"), _V, I("starts"), B, L, nv.PS_RNG_STREAM, I("uniforms"), I("uoff"), 0, 0, 0,
                       I("nodeinfo"), I("guide"), O("paths"), ST], tuple(ins), {"paths": ((B, L), np.int32)}, tuple(exp))


# ---- the device MT19937 stream (csrc/mt19937.hip): numpy is the oracle ------------------------------------------------------------
_MT_POS = 176


@functools.lru_cache(maxsize=None)
def _mt_polys():
    from pinsage_hip import mtjump
    from helpers import mt_cases as mc
    g = mc.GEOM
    assert (lib().ps_mt19937_chunk_log2(), lib().ps_mt19937_window_shift()) == (g.chunk_log2, g.window_shift)
    jp, rp, wp = mtjump.jump_polynomials(), mtjump.radix_polynomials(g.chunk_log2), mtjump.window_polynomials(g.chunk_log2, shift=g.window_shift)
    assert jp.shape == (g.jump_levels, mc.MT_N) and rp.shape == (g.radix_levels, 31, mc.MT_N) and wp.shape == (g.n_window, mc.MT_N)
    return {"jump_polys": _c(jp, np.uint32), "radix_polys": _c(rp, np.uint32), "window_polys": _c(wp, np.uint32)}


def _mt_doubles(seed, skip, n):
    from helpers import mt_cases as mc
    rs = mc.state_at(_MT_POS, seed)
    key = _c(rs.get_state()[1], np.uint32)
    rs.random_sample(skip)
    out = rs.random_sample(n)
    st = rs.get_state()
    return key, {"out": out, "state_out": _c(st[1], np.uint32), "pos_out": np.array([st[2]], np.int32)}


def _mt_sample_case(name, skip, n, parallel):
    from helpers import mt_cases as mc
    g = mc.GEOM
    polys = _mt_polys() if parallel else {}
    ins, exp = [], []
    for seed in (1234, 4321):
        key, e = _mt_doubles(seed, skip, n)
        ins.append(dict(polys, state_in=key))
        exp.append(e)
    assert mc.takes_parallel_path(skip, n, parallel) == parallel
    if parallel:
        assert mc.make_plan(_MT_POS, skip, n).K == 2               # 2 n words: just past one chunk, two workgroups and one window product
        args = [I("state_in"), _MT_POS, skip, n, O("out"), O("state_out"), O("pos_out"), I("jump_polys"), g.jump_levels,
                I("radix_polys"), g.radix_levels, I("window_polys"), g.n_window, WS, WSB, ST]
    else:
        args = [I("state_in"), _MT_POS, skip, n, O("out"), O("state_out"), O("pos_out"), None, 0, None, 0, None, 0, None, 0, ST]
    return Case("ps_mt19937_random_sample", args, tuple(ins),
                {"out": ((n,), np.float64), "state_out": ((mc.MT_N,), np.uint32), "pos_out": ((1,), np.int32)}, tuple(exp),
                ws=("ps_mt19937_workspace_bytes", (skip, n)) if parallel else None)


@case
def _ps_mt19937_random_sample(name):
    """jump, radix and window polynomials, a skipped prefix, 2 n words just past one chunk"""
    return _mt_sample_case(name, 5, (1 << 16) + 37, True)


def _mt_serial(name):
    """the serial form: NULL polynomials and workspace, one workgroup"""
    return _mt_sample_case(name, 0, 3001, False)


@case
def _ps_mt19937_raw_stream(name):
    """the smallest request the raw form serves; the words past the plan's w_hi stay unwritten"""
    from helpers import mt_cases as mc
    g, n = mc.GEOM, (1 << 17) + 3
    p = mc.make_plan(_MT_POS, 0, n)
    assert p.K >= 2 and p.w_hi <= 2 * n + 2 * mc.MT_N
    ins, exp = [], []
    for seed in (1234, 4321):
        key, e = _mt_doubles(seed, 0, n)
        raw = np.full(2 * n + 2 * mc.MT_N, mc.FILL, np.uint32)
        raw[:p.w_hi] = mc.untemper(mc.tempered_words(mc.state_at(_MT_POS, seed), p.w_hi))
        ins.append(dict(_mt_polys(), state_in=key))
        exp.append({"raw": raw, "state_out": e["state_out"], "pos_out": e["pos_out"]})
    return Case(name, [I("state_in"), _MT_POS, n, O("raw"), O("state_out"), O("pos_out"), I("jump_polys"), g.jump_levels,
                       I("radix_polys"), g.radix_levels, I("window_polys"), g.n_window, None, 0, WS, WSB, ST], tuple(ins),
                {"raw": ((2 * n + 2 * mc.MT_N,), np.uint32), "state_out": ((mc.MT_N,), np.uint32), "pos_out": ((1,), np.int32)},
                tuple(exp), ws=("ps_mt19937_workspace_bytes", (0, n)))


# ---- neighbour gathers and their backward (csrc/importance_pool.hip, neigh_agg.hip, neigh_agg_bwd.hip) -----------------------------
def _agg_sets(ci):
    """input set A = agg_bwd_cases.case(ci); set B = its rows in reverse order with rescaled features (the same shapes)"""
    from helpers import agg_bwd_cases as abc
    a = {k: (_c(v) if isinstance(v, np.ndarray) else v) for k, v in abc.case(ci).items()}
    b = dict(a)
    for k, s in (("x", 1.5), ("v", -0.75), ("u", 1.25), ("g", -1.5)):
        b[k] = _c(a[k][::-1] * np.float32(s))
    for k in ("ids", "nvalid", "counts", "wts"):
        b[k] = _c(a[k][::-1])
    b["w2"] = _c(a["w2"][::-1])
    return a, b


def _agg_case(name, ci, args, ins, outs, oracle, ws=None, extra=None):
    sets = _agg_sets(ci)
    inputs, exp = [], []
    for s in sets:
        s = dict(s)
        if extra is not None:
            s.update(extra(s))
        inputs.append({k: s[k] for k in ins})
        exp.append(oracle(s) if oracle is not None else {})
    a = sets[0]
    shapes = {"B": a["B"], "N": a["N"], "H": a["H"], "T": a["T"]}
    return Case(name, args(a), tuple(inputs), outs(shapes), tuple(exp), ws=ws(shapes) if ws else None)


_POOL_CASE = 1            # B = 50, N = 97, H = 64, T = 16: the four-rows-per-wave pooling kernel, 16-byte sweeps


@case
def _ps_importance_pool(name):
    from oracle import c_oracle as co
    return _agg_case(name, _POOL_CASE,
                     lambda a: [I("x"), a["N"], a["H"], I("ids"), I("counts"), None, I("nvalid"), a["B"], a["T"], a["max_idx"], 1, O("out"), ST],
                     ("x", "ids", "counts", "nvalid"), lambda s: {"out": ((s["B"], s["H"]), np.float32)},
                     lambda s: {"out": co.pool_ex(s["x"], s["ids"], s["counts"], None, s["nvalid"], s["max_idx"], True, lanes=16)})


@case
def _ps_pool_weights(name):
    from helpers import agg_bwd_cases as abc
    return _agg_case(name, _POOL_CASE,
                     lambda a: [I("ids"), I("counts"), None, I("nvalid"), a["B"], a["T"], a["max_idx"], 1, 16, O("w_eff"), ST],
                     ("ids", "counts", "nvalid"), lambda s: {"w_eff": ((s["B"], s["T"]), np.float32)},
                     lambda s: {"w_eff": abc.pool_weights_exact(s["ids"], s["counts"], None, s["nvalid"], s["max_idx"], 1, 16)})


@case
def _ps_attention_weights(name):
    """no bit-exact restatement (the softmax's expf): eager expectation"""
    return _agg_case(name, _POOL_CASE,
                     lambda a: [I("u"), I("v"), a["N"], a["H"], I("w2"), I("ids"), I("nvalid"), a["B"], a["T"], O("attn"), ST],
                     ("u", "v", "w2", "ids", "nvalid"), lambda s: {"attn": ((s["B"], s["T"]), np.float32)}, None)


@case
def _ps_gather_max(name):
    from helpers import agg_cases as agc
    return _agg_case(name, _POOL_CASE, lambda a: [I("x"), a["N"], a["H"], I("ids"), I("nvalid"), a["B"], a["T"], O("out"), ST],
                     ("x", "ids", "nvalid"), lambda s: {"out": ((s["B"], s["H"]), np.float32)},
                     lambda s: {"out": agc.gather_max_ref(s["x"], s["ids"], s["nvalid"])})


@case
def _ps_gather_max_arg(name):
    from helpers import agg_bwd_cases as abc
    return _agg_case(name, _POOL_CASE,
                     lambda a: [I("x"), a["N"], a["H"], I("ids"), I("nvalid"), a["B"], a["T"], O("out"), O("arg"), ST],
                     ("x", "ids", "nvalid"), lambda s: {"out": ((s["B"], s["H"]), np.float32), "arg": ((s["B"], s["H"]), np.int32)},
                     lambda s: dict(zip(("out", "arg"), abc.gather_max_arg_ref(s["x"], s["ids"], s["nvalid"]))))


def _slot_lists(s):
    from helpers import agg_bwd_cases as abc
    rptr, slots = abc.slot_lists_ref(s["ids"], abc.kept_pool(s["ids"], s["nvalid"], s["max_idx"]), s["N"])
    assert np.diff(rptr).max() > abc.segment() and (np.diff(rptr) == 0).any()          # a hub row that is cut, and an empty row
    return rptr, slots


@case
def _ps_gather_bwd(name):
    """the hub batch: one feature row named by more than ps_gather_bwd_segment() slots -- both launches and the workspace"""
    from helpers import agg_bwd_cases as abc

    def extra(s):
        rptr, slots = _slot_lists(s)
        coef = abc.pool_weights_exact(s["ids"], None, s["wts"], s["nvalid"], s["max_idx"], 1, 16)
        return {"rptr": rptr, "slots": slots, "coef": _c(coef.reshape(-1))}
    return _agg_case(name, abc.HUB_CASE,
                     lambda a: [I("rptr"), I("slots"), a["N"], a["T"], I("coef"), None, I("g"), a["B"], a["H"], O("gx"), WS, WSB, ST],
                     ("rptr", "slots", "coef", "g"), lambda s: {"gx": ((s["N"], s["H"]), np.float32)},
                     lambda s: {"gx": abc.gather_bwd_exact(s["rptr"], s["slots"], s["N"], s["T"], s["g"], coef=s["coef"])},
                     ws=lambda s: ("ps_gather_bwd_workspace_bytes", (s["B"], s["T"], s["H"])), extra=extra)


@case
def _ps_attention_bwd_cols(name):
    from helpers import agg_bwd_cases as abc

    def extra(s):
        rptr, slots = _slot_lists(s)
        ds = np.random.RandomState(int(abs(s["g"][0, 0]) * 1000) + 5).standard_normal(s["B"] * s["T"]).astype(np.float32)
        return {"rptr": rptr, "slots": slots, "ds": ds}
    return _agg_case(name, abc.HUB_CASE,
                     lambda a: [I("rptr"), I("slots"), a["N"], a["T"], I("ds"), I("u"), I("v"), a["H"], I("w2"), a["B"], O("dv"), WS, WSB, ST],
                     ("rptr", "slots", "ds", "u", "v", "w2"), lambda s: {"dv": ((s["N"], s["H"]), np.float32)},
                     lambda s: {"dv": abc.attention_bwd_cols_exact(s["rptr"], s["slots"], s["N"], s["T"], s["ds"], s["u"], s["v"], s["w2"])},
                     ws=lambda s: ("ps_gather_bwd_workspace_bytes", (s["B"], s["T"], s["H"])), extra=extra)


@case
def _ps_attention_bwd_rows(name):
    from helpers import agg_bwd_cases as abc
    from helpers import agg_cases as agc

    def extra(s):
        return {"attn": agc.attention_weights_ref(s["u"], s["v"], s["w2"], s["ids"], s["nvalid"]).astype(np.float32)}

    def oracle(s):
        ds, du, dw2, _ = abc.attention_bwd_rows_exact(s["x"], s["u"], s["v"], s["w2"], s["ids"], s["nvalid"], s["attn"], s["g"], s["vec"])
        return {"ds": ds, "du": du, "dw2": dw2}
    return _agg_case(name, _POOL_CASE,
                     lambda a: [I("x"), a["N"], a["H"], I("u"), I("v"), a["H"], I("w2"), I("ids"), I("nvalid"), I("attn"), I("g"), a["B"],
                                a["T"], O("ds"), O("du"), O("dw2"), WS, WSB, ST],
                     ("x", "u", "v", "w2", "ids", "nvalid", "attn", "g"),
                     lambda s: {"ds": ((s["B"], s["T"]), np.float32), "du": ((s["B"], s["H"]), np.float32), "dw2": ((s["H"],), np.float32)},
                     oracle, ws=lambda s: ("ps_attention_bwd_rows_workspace_bytes", (s["B"], s["H"])), extra=extra)


# ---- batch norm (csrc/batch_norm.hip) ------------------------------------------------------------------------------------------------
def _bn_sets():
    """bn_cases' "ragged-steps" data (M = 161: two partitions of the workspace, N = 8: 16-byte sweeps) and a second set from it"""
    from helpers import bn_cases as bc
    d = bc.stats_data("ragged-steps")
    a = {"z": _c(d["z"]), "gamma": _c(d["gamma"])}
    b = {"z": _c(d["z"][::-1] * np.float32(1.25) + np.float32(0.5)), "gamma": _c(d["gamma"][::-1])}
    return d, a, b


@case
def _ps_bn_batch_stats(name):
    from helpers import bn_cases as bc
    d, a, b = _bn_sets()
    M, N = d["M"], d["N"]
    assert bc.stats_facts(M, N)["P"] >= 2
    exp = []
    for s in (a, b):
        e = bc.stats_exact(s["z"], s["gamma"], d["rm0"], d["rv0"])
        assert all(e["decided"][k].all() for k in bc.OUTPUTS), name       # every bit follows from the header's arithmetic
        exp.append({"mean": e["mean"], "var": e["var"], "scale": e["scale"], "running_mean": e["rm"], "running_var": e["rv"]})
    return Case(name, [I("z"), M, N, I("gamma"), float(bc.EPS), float(bc.MOMENTUM), IO("running_mean"), IO("running_var"), O("mean"),
                       O("var"), O("scale"), WS, WSB, ST], (a, b), {k: ((N,), np.float32) for k in ("mean", "var", "scale")}, tuple(exp),
                inout={"running_mean": _c(d["rm0"]), "running_var": _c(d["rv0"])}, ws=("ps_bn_stats_workspace_bytes", (M, N)))


@case
def _ps_bn_apply(name):
    from helpers import bn_cases as bc
    from pinsage_hip import native as nv
    d, a, b = _bn_sets()
    M, N = d["M"], d["N"]
    rs = np.random.RandomState(77)
    ins, exp = [], []
    for s in (a, b):
        e = bc.stats_exact(s["z"], s["gamma"])
        s = {"z": s["z"], "mean": e["mean"], "scale": e["scale"], "beta": (0.5 * rs.standard_normal(N)).astype(np.float32)}
        ins.append(s)
        exp.append({"y": bc.apply_exact(s["z"], s["mean"], s["scale"], s["beta"], True, True, bc.apply_facts(M, N)["vec"])})
    return Case(name, [I("z"), M, N, I("mean"), I("scale"), I("beta"), nv.PS_RELU | nv.PS_L2NORM, O("y"), ST], tuple(ins),
                {"y": ((M, N), np.float32)}, tuple(exp))


# ---- dense layers (csrc/dense_mfma.hip) ------------------------------------------------------------------------------------------
@case
def _ps_permute_k(name):
    """the header's one line restated: every group of eight k as k 0 2 4 6 1 3 5 7; W is a column slice (ld > K)"""
    rows, K, ld = 37, 40, 48
    ins, exp = [], []
    for seed in (1, 2):
        big = np.random.RandomState(seed).standard_normal((rows, ld)).astype(np.float32)
        ins.append({"W": big})
        exp.append({"out": _c(big[:, :K].reshape(rows, K // 8, 8)[:, :, [0, 2, 4, 6, 1, 3, 5, 7]].reshape(rows, K))})
    return Case(name, [I("W"), rows, K, ld, O("out"), ST], tuple(ins), {"out": ((rows, K), np.float32)}, tuple(exp))


@case
def _ps_linear(name):
    """both operand pairs, bias, ReLU: the C oracle's fmaf chain bit for bit (the row norm has only a bound: not used here)"""
    from oracle import c_oracle as co
    from pinsage_hip import native as nv
    M, K, N, K2 = 70, 40, 33, 24
    ins, exp = [], []
    for seed in (1, 2):
        rs = np.random.RandomState(seed)
        s = {"x": rs.standard_normal((M, K)), "W": rs.standard_normal((N, K)) / 6, "b": rs.standard_normal(N),
             "x2": rs.standard_normal((M, K2)), "W2": rs.standard_normal((N, K2)) / 5}
        s = {k: _c(v, np.float32) for k, v in s.items()}
        ins.append(s)
        exp.append({"y": co.linear(s["x"], s["W"], s["b"], x2=s["x2"], W2=s["W2"], relu=True)})
    return Case(name, [I("x"), M, K, I("W"), K, I("b"), N, I("x2"), K2, I("W2"), K2, nv.PS_RELU, O("y"), ST], tuple(ins),
                {"y": ((M, N), np.float32)}, tuple(exp))


_GCN_CASE = "k32h64-T5-64j+1-counts"       # the smallest served shape: ragged M just above 64 * 384, one mixed tile


def _gcn_sets():
    from helpers import gcn_cases as gc
    c = next(c for c in gc.FUSED_CASES if c.name == _GCN_CASE)
    d = gc.gcn_data(c)
    assert gc.gcn_served(c.M, c.K, gc.N_OUT, c.H, c.T) and c.form == "counts"
    a = {"x": _c(d.x), "W": _c(d.W), "b": _c(d.b), "h_full": _c(d.h_full), "ids": _c(d.rows.ids, np.int32),
         "counts": _c(d.rows.counts, np.int32), "nvalid": _c(d.rows.nvalid, np.int32), "W2": _c(d.W2)}
    b = dict(a, x=_c(a["x"][::-1] * np.float32(1.5)), h_full=_c(a["h_full"] * np.float32(-0.75)), b=_c(a["b"][::-1]))
    return c, d, a, b


def _gcn_args(c, d, tail):
    from helpers import gcn_cases as gc
    from pinsage_hip import native as nv
    return [I("x"), c.M, c.K, I("W"), c.K, I("b"), gc.N_OUT, I("h_full"), d.n_full, c.H, I("ids"), I("counts"), None, I("nvalid"), c.T,
            int(d.max_idx_arg), 1, I("W2"), c.H, nv.PS_RELU | nv.PS_L2NORM, O("y"), WS, WSB] + tail + [ST]


@case
def _ps_gcn_layer(name):
    """eager expectation: after the row norm the oracle gives a bound, not bits"""
    from helpers import gcn_cases as gc
    c, d, a, b = _gcn_sets()
    return Case(name, _gcn_args(c, d, []), (a, b), {"y": ((c.M, gc.N_OUT), np.float32)}, ({}, {}),
                ws=("ps_gcn_layer_workspace_bytes", (c.M, c.H)))


def _gcn_keeps(ids, nvalid, T, max_idx):
    from helpers import gcn_cases as gc
    return gc.row_keeps(ids.astype(np.int64), nvalid.astype(np.int64), T, max_idx)


@case
def _ps_gcn_layer_ordered(name):
    """eager expectation as for ps_gcn_layer; the row order it is given is the numpy restatement's"""
    from helpers import gcn_cases as gc
    from helpers import gcn_order as go
    c, d, a, b = _gcn_sets()
    ord_, heavy = go.chunk_partition(_gcn_keeps(a["ids"], a["nvalid"], c.T, min(d.max_idx_arg, d.n_full - 1)))
    assert heavy.any() and not heavy.all()
    a, b = dict(a, ord=ord_, tile_heavy=heavy), dict(b, ord=ord_, tile_heavy=heavy)
    return Case(name, _gcn_args(c, d, [I("ord"), I("tile_heavy")]), (a, b), {"y": ((c.M, gc.N_OUT), np.float32)}, ({}, {}),
                ws=("ps_gcn_layer_workspace_bytes", (c.M, c.H)))


@case
def _ps_gcn_order(name):
    """two layers in one launch; the second input set has them swapped"""
    from helpers import gcn_order as go
    c, d, a, _ = _gcn_sets()
    max_idx = min(d.max_idx_arg, d.n_full - 1)
    l0 = (a["ids"], a["nvalid"])
    l1 = (_c(a["ids"][::-1]), _c(a["nvalid"][::-1]))
    ins, exp = [], []
    for layers in ((l0, l1), (l1, l0)):
        ins.append({"ids": _c(np.stack([l[0] for l in layers])), "nvalid": _c(np.stack([l[1] for l in layers]))})
        parts = [go.chunk_partition(_gcn_keeps(l[0], l[1], c.T, max_idx)) for l in layers]
        exp.append({"ord": _c(np.stack([p[0] for p in parts])), "tile_heavy": _c(np.stack([p[1] for p in parts]))})
    nt = -(-c.M // go.TILE)
    assert c.M > go.CHUNK and c.M % go.TILE
    return Case(name, [I("ids"), I("nvalid"), 2, c.M, c.T, int(max_idx), O("ord"), O("tile_heavy"), ST], tuple(ins),
                {"ord": ((2, nt * go.TILE), np.int32), "tile_heavy": ((2, nt), np.int32)}, tuple(exp))


# ---- LSH codes, Hamming search (csrc/lsh_filter.hip, hamming_topk.hip, hamming_mfma.hip) -------------------------------------------
_LSH_N, _LSH_D, _LSH_BITS = 200, 32, 64


def _lsh_sets():
    sets = []
    for seed in (21, 22):
        rs = np.random.RandomState(seed)
        sets.append({"x": rs.standard_normal((_LSH_N, _LSH_D)).astype(np.float32),
                     "A": rs.standard_normal((_LSH_BITS, _LSH_D)).astype(np.float32)})
    return sets


def _stage_bytes():
    n = int(lib().ps_lsh_stage_bytes(_LSH_BITS, _LSH_D))
    assert n > 0, "the staged path does not serve the case's shape"
    return n


@case
def _ps_lsh_stage(name):
    """no restatement of the staged image: eager expectation"""
    n = _stage_bytes()
    a, b = ({"A": s["A"]} for s in _lsh_sets())
    return Case(name, [I("A"), _LSH_BITS, _LSH_D, O("staged"), n, ST], (a, b), {"staged": ((n,), np.uint8)}, ({}, {}))


def _staged_inputs():
    """the x of both input sets with a placeholder for the image, which the GPU test takes from ps_lsh_stage's case"""
    n = _stage_bytes()
    return tuple({"x": s["x"], "staged": np.zeros(n, np.uint8) + np.uint8(i)} for i, s in enumerate(_lsh_sets()))


@case
def _ps_lsh_encode(name):
    """the staged path (bf16 filter, exact recheck): the image is ps_lsh_stage's output for the same A"""
    from oracle import c_oracle as co
    from pinsage_hip import native as nv
    exp = tuple({"codes": co.lsh_encode(s["x"], s["A"])} for s in _lsh_sets())
    return Case(name, [I("x"), _LSH_N, _LSH_D, I("staged"), _LSH_BITS, O("codes"), nv.PS_LSH_STAGED, ST], _staged_inputs(),
                {"codes": ((_LSH_N, _LSH_BITS // 8), np.uint8)}, exp, derived={"staged": ("ps_lsh_stage", "staged")})


@case
def _ps_lsh_encode_planes(name):
    """codes from the C oracle; the planes have no restatement: eager expectation"""
    from oracle import c_oracle as co
    n = int(lib().ps_lsh_planes_bytes(_LSH_N, _LSH_BITS // 8))
    assert n > 0
    exp = tuple({"codes": co.lsh_encode(s["x"], s["A"])} for s in _lsh_sets())
    return Case(name, [I("x"), _LSH_N, _LSH_D, I("staged"), _LSH_BITS, O("codes"), O("planes"), ST], _staged_inputs(),
                {"codes": ((_LSH_N, _LSH_BITS // 8), np.uint8), "planes": ((n,), np.uint8)}, exp,
                derived={"staged": ("ps_lsh_stage", "staged")})


_HAM_NQ, _HAM_N, _HAM_CS, _HAM_K, _HAM_OFF = 64, 4096, 8, 10, 1000      # the smallest shape the MFMA scan serves


def _ham_sets():
    sets = []
    for seed in (31, 32):
        rs = np.random.RandomState(seed)
        sets.append({"codes": rs.randint(0, 256, (_HAM_N, _HAM_CS)).astype(np.uint8),
                     "qcodes": rs.randint(0, 256, (_HAM_NQ, _HAM_CS)).astype(np.uint8)})
    return sets


def _ham_expect():
    from oracle import c_oracle as co
    out = []
    for s in _ham_sets():
        d, i = co.hamming_topk(s["qcodes"], s["codes"], _HAM_K, id_offset=_HAM_OFF)
        out.append({"dist": d.astype(np.int32), "ids": i})
    return tuple(out)


_HAM_OUT = {"dist": ((_HAM_NQ, _HAM_K), np.int32), "ids": ((_HAM_NQ, _HAM_K), np.int64)}


@case
def _ps_lsh_expand(name):
    """no restatement of the plane layout: eager expectation"""
    n = int(lib().ps_lsh_planes_bytes(_HAM_N, _HAM_CS))
    assert n == 4 * _HAM_N * _HAM_CS
    a, b = ({"codes": s["codes"]} for s in _ham_sets())
    return Case(name, [I("codes"), _HAM_N, _HAM_CS, O("planes"), ST], (a, b), {"planes": ((n,), np.uint8)}, ({}, {}))


@case
def _ps_hamming_topk(name):
    return Case(name, [I("qcodes"), _HAM_NQ, I("codes"), _HAM_N, _HAM_CS, _HAM_K, _HAM_OFF, O("dist"), O("ids"), WS, WSB, ST],
                tuple(_ham_sets()), _HAM_OUT, _ham_expect(), ws=("ps_hamming_topk_workspace_bytes", (_HAM_NQ, _HAM_N, _HAM_CS, _HAM_K)))


def _ham_mfma(name, query, qn):
    """the smallest table the scan serves (half of it is refused), and the plan cuts it into two or more slices: the merge runs"""
    slices = lib().ps_debug_hm_slices                              # the plan's own count (an export outside the header, for tests)
    slices.restype, slices.argtypes = ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    assert slices(_HAM_NQ, _HAM_N, _HAM_CS, _HAM_K) >= 2 and slices(_HAM_NQ, _HAM_N // 2, _HAM_CS, _HAM_K) == 0
    n = int(lib().ps_lsh_planes_bytes(_HAM_N, _HAM_CS))
    ins = []
    for i, s in enumerate(_ham_sets()):
        d = {"dbplanes": np.zeros(n, np.uint8) + np.uint8(i)}
        d[query] = s["qcodes"] if query == "qcodes" else np.zeros(qn, np.uint8) + np.uint8(i)
        ins.append(d)
    derived = {"dbplanes": ("ps_lsh_expand", "planes")}
    if query == "qplanes":
        derived["qplanes"] = ("ps_lsh_expand:queries", "planes")
    return Case(name, [I(query), _HAM_NQ, I("dbplanes"), _HAM_N, _HAM_CS, _HAM_K, _HAM_OFF, O("dist"), O("ids"), WS, WSB, ST], tuple(ins),
                _HAM_OUT, _ham_expect(), ws=("ps_hamming_topk_mfma_workspace_bytes", (_HAM_NQ, _HAM_N, _HAM_CS, _HAM_K)), derived=derived)


@case
def _ps_hamming_topk_mfma(name):
    return _ham_mfma(name, "qplanes", int(lib().ps_lsh_planes_bytes(_HAM_NQ, _HAM_CS)))


@case
def _ps_hamming_topk_mfma_codes(name):
    return _ham_mfma(name, "qcodes", 0)


def _expand_queries(name):
    """ps_lsh_expand over the queries of the Hamming cases (the planes ps_hamming_topk_mfma is given)"""
    n = int(lib().ps_lsh_planes_bytes(_HAM_NQ, _HAM_CS))
    a, b = ({"codes": s["qcodes"]} for s in _ham_sets())
    return Case(name, [I("codes"), _HAM_NQ, _HAM_CS, O("planes"), ST], (a, b), {"planes": ((n,), np.uint8)}, ({}, {}))


def _merge_sets(P=3, per=200, nq=9, k=7):
    from oracle import c_oracle as co
    sets = []
    for seed in (41, 42):
        rs = np.random.RandomState(seed)
        codes = rs.randint(0, 4, (P * per, 8)).astype(np.uint8)            # few distinct codes: ties across the shards
        q = rs.randint(0, 4, (nq, 8)).astype(np.uint8)
        parts = [co.hamming_topk(q, codes[p * per:(p + 1) * per], k, id_offset=p * per) for p in range(P)]
        d, i = co.hamming_topk(q, codes, k)
        sets.append((np.stack([x[0] for x in parts]).astype(np.int32), np.stack([x[1] for x in parts]),
                     {"dist": d.astype(np.int32), "ids": i}))
    return P, nq, k, sets


@case
def _ps_topk_merge(name):
    """the shards' lists and the merged list are both the C oracle's (the search over a part / over the whole table)"""
    P, nq, k, sets = _merge_sets()
    return Case(name, [I("dist_in"), I("ids_in"), P, nq, k, O("dist"), O("ids"), ST],
                tuple({"dist_in": _c(s[0]), "ids_in": _c(s[1])} for s in sets),
                {"dist": ((nq, k), np.int32), "ids": ((nq, k), np.int64)}, tuple(s[2] for s in sets))


@case
def _ps_topk_merge_strided(name):
    P, nq, k, sets = _merge_sets()
    ds, is_ = nq * k + 5, nq * k + 3
    ins = []
    for d, i, _ in sets:
        dd, ii = np.full((P, ds), 7, np.int32), np.full((P, is_), -9, np.int64)
        dd[:, :nq * k], ii[:, :nq * k] = d.reshape(P, -1), i.reshape(P, -1)
        ins.append({"dist_in": dd, "ids_in": ii})
    return Case(name, [I("dist_in"), ds, I("ids_in"), is_, P, nq, k, O("dist"), O("ids"), ST], tuple(ins),
                {"dist": ((nq, k), np.int32), "ids": ((nq, k), np.int64)}, tuple(s[2] for s in sets))


# ---- exact searches (csrc/dot_topk.hip): topk_cases' planted tables and oracle ------------------------------------------------------
def _topk_pair(case_name):
    """(case A of topk_cases, a case B of the same shape with the table reversed and shifted, their oracles)"""
    from helpers import topk_cases as tc
    a = tc.cases()[case_name]
    kw = {k: v for k, v in a.__dict__.items() if k not in ("name", "kind", "k", "D", "x", "N", "nq")}
    b = tc.Case(a.name + "-reversed", a.kind, a.x[::-1] + 1, a.k, D=a.D, **kw)
    tc.assert_exact(a), tc.assert_exact(b)
    return a, b, tuple(np.array(x) for x in tc.oracle(a)), tuple(np.array(x) for x in tc.oracle_of(b))


@case
def _ps_dot_topk(name):
    a, b, ea, eb = _topk_pair("dot-regimes-N1500-k100")
    return Case(name, [I("E"), a.N, a.D, I("qidx"), a.nq, a.k, 0, O("vals"), O("ids"), WS, WSB, ST],
                tuple({"E": c.table(), "qidx": _c(c.qidx, np.int64)} for c in (a, b)),
                {"vals": ((a.nq, a.k), np.float32), "ids": ((a.nq, a.k), np.int64)},
                tuple({"vals": e[0], "ids": e[1]} for e in (ea, eb)), ws=("ps_dot_topk_workspace_bytes", (a.nq, a.N, a.D, a.k)))


@case
def _ps_l2_topk(name):
    """the masked form: assign and probe words given"""
    from helpers import topk_cases as tc
    a, b, ea, eb = _topk_pair("l2m-improving-N1500-nlist70-k40")
    words = tc.probe_bits(a).shape[1]
    return Case(name, [I("X"), a.N, a.D, I("Q"), a.nq, a.k, I("assign"), I("probe"), words, O("dist"), O("ids"), WS, WSB, ST],
                tuple({"X": c.table(), "Q": c.queries(), "assign": _c(c.assign, np.int32), "probe": tc.probe_bits(c)} for c in (a, b)),
                {"dist": ((a.nq, a.k), np.float32), "ids": ((a.nq, a.k), np.int64)},
                tuple({"dist": e[0], "ids": e[1]} for e in (ea, eb)), ws=("ps_l2_topk_workspace_bytes", (a.nq, a.N, a.D, a.k)))


@case
def _ps_ivf_topk(name):
    a, b, ea, eb = _topk_pair("ivf-p3-k40")
    nprobe = a.probes.shape[1]
    return Case(name, [I("X"), a.N, a.D, I("list_ptr"), a.nlist, a.max_list, I("item_ids"), I("Q"), a.nq, I("probes"), nprobe, a.k,
                       O("dist"), O("ids"), WS, WSB, ST],
                tuple({"X": c.table(), "list_ptr": _c(c.list_ptr, np.int64), "item_ids": _c(c.item_ids, np.int64), "Q": c.queries(),
                       "probes": _c(c.probes, np.int32)} for c in (a, b)),
                {"dist": ((a.nq, a.k), np.float32), "ids": ((a.nq, a.k), np.int64)},
                tuple({"dist": e[0], "ids": e[1]} for e in (ea, eb)),
                ws=("ps_ivf_topk_workspace_bytes", (a.nq, a.N, a.D, a.k, a.nlist, nprobe, a.max_list)))


def _rank_sets():
    from oracle import c_oracle as co
    N, D, nq, off = 300, 24, 40, 5000
    sets = []
    for seed in (51, 52):
        rs = np.random.RandomState(seed)
        E = rs.randint(-3, 4, (N, D)).astype(np.float32)          # small integers: many equal similarities, the id decides
        Q = rs.randint(-3, 4, (nq, D)).astype(np.float32)
        t = rs.randint(0, N, nq).astype(np.int64)
        sim = co.linear(Q, E)
        sets.append(dict(E=E, Q=Q, t=t, sim=sim, thr=_c(sim[np.arange(nq), t]), tid=_c(t + off)))
    return N, D, nq, off, sets


@case
def _ps_row_dot(name):
    """out[i] is the entry of the C oracle's GEMM for the pair"""
    N, D, nq, _, sets = _rank_sets()
    ia = np.arange(nq, dtype=np.int64)[::-1].copy()
    return Case(name, [I("A"), nq, I("B"), N, D, I("ia"), I("ib"), nq, O("out"), ST],
                tuple({"A": s["Q"], "B": s["E"], "ia": ia, "ib": s["t"]} for s in sets), {"out": ((nq,), np.float32)},
                tuple({"out": _c(s["sim"][ia, s["t"]])} for s in sets))


@case
def _ps_rank_count(name):
    """count is ADDED to: an in-out buffer that starts from non-zero values"""
    N, D, nq, off, sets = _rank_sets()
    init = np.arange(nq, dtype=np.int64) * 3 + 1
    exp = []
    for s in sets:
        ids = off + np.arange(N)
        before = (s["sim"] > s["thr"][:, None]) | ((s["sim"] == s["thr"][:, None]) & (ids[None, :] < s["tid"][:, None]))
        exp.append({"count": init + before.sum(axis=1)})
    assert any((e["count"] - init).max() > 10 for e in exp)
    return Case(name, [I("E"), N, D, off, I("Q"), nq, I("thr"), I("tid"), IO("count"), ST],
                tuple({k: s[k] for k in ("E", "Q", "thr", "tid")} for s in sets), {}, tuple(exp), inout={"count": init})


# ---- SpMM / SDDMM (csrc/spmm_csr.hip, spmm_exact.hip): spmm_cases' restatement -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spmm_sets():
    """spmm_cases' "straddle" graph: E > S with one row across slot S; the second set has the features reversed and val negated"""
    from helpers import spmm_cases as sc
    c = sc.case("straddle")
    S = c["S"]
    assert c["E"] > S and any(len(p) > 1 for p in sc.pieces(c["rowptr"], S))
    # no row spans more than two slices: a cut row of ps_spmm_csr is two addends onto +0.0, whose sum does not depend on their order
    assert max(len(p) for p in sc.pieces(c["rowptr"], S)) == 2
    a = {k: _c(c[k]) for k in ("rowptr", "col", "val", "x", "g")}
    b = dict(a, val=_c(-a["val"]), x=_c(a["x"][::-1]), g=_c(a["g"][::-1] * np.float32(0.5)))
    return c, a, b


@case
def _ps_spmm_csr(name):
    from helpers import spmm_cases as sc
    c, a, b = _spmm_sets()
    ins = ("rowptr", "col", "val", "x")
    return Case(name, [I("rowptr"), I("col"), I("val"), I("x"), c["N"], c["H"], c["V"], c["E"], O("out"), ST],
                tuple(_pick(s, *ins) for s in (a, b)), {"out": ((c["V"], c["H"]), np.float32)},
                tuple({"out": sc.spmm_exact(s["rowptr"], s["col"], s["val"], s["x"], c["S"])} for s in (a, b)))


@case
def _ps_spmm_csr_exact(name):
    from helpers import spmm_cases as sc
    c, a, b = _spmm_sets()
    ins = ("rowptr", "col", "val", "x")
    return Case(name, [I("rowptr"), I("col"), I("val"), I("x"), c["N"], c["H"], c["V"], c["E"], O("out"), WS, WSB, ST],
                tuple(_pick(s, *ins) for s in (a, b)), {"out": ((c["V"], c["H"]), np.float32)},
                tuple({"out": sc.spmm_exact(s["rowptr"], s["col"], s["val"], s["x"], c["S"])} for s in (a, b)),
                ws=("ps_spmm_csr_exact_workspace_bytes", (c["E"], c["H"])))


@case
def _ps_sddmm_csr(name):
    from helpers import spmm_cases as sc
    c, a, b = _spmm_sets()
    ins = ("rowptr", "col", "x", "g")
    return Case(name, [I("rowptr"), I("col"), I("x"), c["N"], I("g"), c["V"], c["H"], c["E"], O("d"), ST],
                tuple(_pick(s, *ins) for s in (a, b)), {"d": ((c["E"],), np.float32)},
                tuple({"d": sc.sddmm_exact(s["rowptr"], s["col"], s["x"], s["g"], c["vec"])} for s in (a, b)))


# ---- ranking losses (csrc/loss.hip): loss_cases' data, the C oracle --------------------------------------------------------------
_LOSS_MARGIN, _LOSS_GO = 0.1, 0.3


@functools.lru_cache(maxsize=None)
def _loss_sets():
    """shared candidates, B = 65 (a second ballot of one row), N = 37, D = 36: the two data kinds of loss_cases as the two sets"""
    from oracle import c_oracle as co
    from helpers import loss_cases as lc
    sets = []
    for kind in ("unit", "levels"):
        c = lc.BY_NAME[f"shared-B65-N37-D36-{kind}"]
        d = lc.loss_data(c)
        s = {"Q": _c(d.Q), "P": _c(d.P), "X": _c(d.X)}
        s["sim"], s["idx"] = co.hardest_negative(s["Q"], s["X"])
        s["row_loss"], s["active"], loss = co.margin_loss(s["Q"], s["P"], s["sim"], _LOSS_MARGIN)
        s["loss"] = np.array([loss], np.float32)
        s["grad_out"] = np.array([_LOSS_GO], np.float32)
        s.update(co.margin_loss_bwd(s["Q"], s["P"], s["X"], lc.SHARED, s["idx"], s["active"], np.float32(_LOSS_GO)))
        assert s["active"].any() and not s["active"].all()
        sets.append(s)
    return c.B, c.N, c.D, sets


@case
def _ps_hardest_negative(name):
    """sim / idx from the C oracle; the packed word `best` has no restatement: eager expectation"""
    B, N, D, sets = _loss_sets()
    return Case(name, [I("Q"), B, D, I("X"), N, 0, O("best"), O("sim"), O("idx"), ST], tuple(_pick(s, "Q", "X") for s in sets),
                {"best": ((B,), np.uint64), "sim": ((B,), np.float32), "idx": ((B,), np.int64)}, tuple(_pick(s, "sim", "idx") for s in sets))


@case
def _ps_margin_loss(name):
    B, N, D, sets = _loss_sets()
    ins = tuple(dict(_pick(s, "Q", "P"), best=np.zeros(B, np.uint64) + np.uint64(i)) for i, s in enumerate(sets))
    outs = ("row_loss", "idx", "active", "loss")
    return Case(name, [I("Q"), I("P"), B, D, I("best"), float(np.float32(_LOSS_MARGIN)), O("row_loss"), O("idx"), O("active"), O("loss"), ST],
                ins, {k: (sets[0][k].shape, sets[0][k].dtype) for k in outs}, tuple(_pick(s, *outs) for s in sets),
                derived={"best": ("ps_hardest_negative", "best")})


@case
def _ps_margin_loss_bwd(name):
    from helpers import loss_cases as lc
    B, N, D, sets = _loss_sets()
    ins, outs = ("Q", "P", "X", "idx", "active", "grad_out"), ("dQ", "dP", "dX")
    return Case(name, [I("Q"), I("P"), I("X"), B, N, D, lc.SHARED, I("idx"), I("active"), I("grad_out"), O("dQ"), O("dP"), O("dX"), ST],
                tuple(_pick(s, *ins) for s in sets), {k: (sets[0][k].shape, sets[0][k].dtype) for k in outs},
                tuple(_pick(s, *outs) for s in sets))


# ---- personalized PageRank (csrc/ppr_push.hip): ppr_cases' restatement of the reference's loop ------------------------------------
@functools.lru_cache(maxsize=None)
def _ppr_sets():
    """ppr_cases' "random" graph (self-loops, duplicate edges, sinks, an isolated node, a source beyond V), ten sweeps; the second
    input set carries the edge weights in reverse order: the same structure, other shares"""
    from helpers import ppr_cases as pc
    ei, ew, sources, alpha, sweeps, k = pc.case("random")
    V = pc.num_nodes("random")
    Vp = pc.size_of("random")
    S, Sc = len(sources), -(-len(sources) // 64) * 64
    assert sweeps >= 2 and Vp > V
    sets = []
    for w in (ew, ew[::-1]):
        adj = [[] for _ in range(V)]
        for e in range(ei.shape[1]):
            adj[int(ei[0, e])].append((int(ei[1, e]), float(w[e])))
        rowptr = np.concatenate([[0], np.cumsum([len(r) for r in adj])]).astype(np.int64)
        inn = pc.in_edges(adj, V)
        summed = [[(u, s) for u, s in row if u > v] + [(u, s) for u, s in row if u < v] for v, row in enumerate(inn)]
        lev = np.array(pc.levels(adj, V))
        score = np.zeros((Vp, Sc))
        for j, src in enumerate(sources):
            score[:, j] = pc.reference_scores(adj, Vp, src, alpha, sweeps)
        rows = _c(score[:, :S].T)
        top = [pc.select(rows[j], k) for j in range(S)]
        ids, sc, wt = np.full((S, k), -1, np.int32), np.zeros((S, k)), np.zeros((S, k))
        for j, (t, wj) in enumerate(top):
            ids[j, :len(t)], sc[j, :len(t)], wt[j, :len(t)] = t, rows[j][t], wj
        sets.append(dict(rowptr=rowptr, wsorted=np.array([x for r in adj for _, x in r], np.float64),
                         share=np.array([x for r in pc.shares(adj) for x in r], np.float64),
                         in_rowptr=np.concatenate([[0], np.cumsum([len(r) for r in summed])]).astype(np.int64),
                         in_src=np.array([u for r in summed for u, _ in r], np.int32),
                         in_share=np.array([s for r in summed for _, s in r], np.float64),
                         level_nodes=_c(np.argsort(lev, kind="stable"), np.int32),
                         level_ptr=np.concatenate([[0], np.cumsum(np.bincount(lev))]).astype(np.int64),
                         sources=np.array(sources, np.int64), score=score, rows=rows, ids=ids, scores=sc, wts=wt,
                         nvalid=np.array([len(t) for t, _ in top], np.int32)))
    a, b = sets
    assert np.array_equal(a["level_ptr"], b["level_ptr"]) and len(a["level_ptr"]) > 2
    assert (a["nvalid"] == k).any() and (a["nvalid"] < k).any()
    return dict(V=V, Vp=Vp, S=S, Sc=Sc, alpha=alpha, sweeps=sweeps, k=k), sets


@case
def _ps_ppr_shares(name):
    p, sets = _ppr_sets()
    return Case(name, [I("rowptr"), I("wsorted"), p["V"], O("share"), ST], tuple(_pick(s, "rowptr", "wsorted") for s in sets),
                {"share": (sets[0]["share"].shape, np.float64)}, tuple(_pick(s, "share") for s in sets))


@case
def _ps_ppr_push(name):
    """ten sweeps, one launch per level and sweep; h_level_ptr is a HOST array, read while the call enqueues"""
    p, sets = _ppr_sets()
    ins = ("in_rowptr", "in_src", "in_share", "level_nodes", "sources")
    n_levels = len(sets[0]["level_ptr"]) - 1
    return Case(name, [I("in_rowptr"), I("in_src"), I("in_share"), p["V"], p["Vp"], I("level_nodes"), HI("h_level_ptr"), n_levels,
                       I("sources"), p["S"], _alpha_bits(p["alpha"]), p["sweeps"], 0, O("score"), WS, WSB, ST],
                tuple(_pick(s, *ins) for s in sets), {"score": ((p["Vp"], p["Sc"]), np.float64)}, tuple(_pick(s, "score") for s in sets),
                host={"h_level_ptr": sets[0]["level_ptr"]}, ws=("ps_ppr_push_workspace_bytes", (p["Vp"], p["S"])))


@case
def _ps_ppr_topk(name):
    p, sets = _ppr_sets()
    outs = ("ids", "scores", "wts", "nvalid")
    return Case(name, [I("rows"), p["S"], p["Vp"], p["Vp"], -1, p["k"], O("ids"), O("scores"), O("wts"), O("nvalid"), ST],
                tuple({"rows": s["rows"]} for s in sets), {k: (sets[0][k].shape, sets[0][k].dtype) for k in outs},
                tuple(_pick(s, *outs) for s in sets))


# ---- item co-occurrence graph (csrc/cooc_mfma.hip, cooc_sparse.hip): cooc_defs' five rules -----------------------------------------
_COOC_THR = 2


@functools.lru_cache(maxsize=None)
def _cooc_sets():
    """700 users (two PS_COOC_WINDOW windows), 40 items, multiplicities up to 3; the second input set renames the items by a fixed
    permutation: the same number of rows, entries and pairs.  The grouped arrays are the package's own host-side preparation
    (pinsage_hip.cooc._Prep, torch on the CPU); everything expected comes from cooc_defs."""
    import torch
    from pinsage_hip import cooc
    # top-level modules, as tests/test_hip_cooc.py and test_hip_cooc_sparse.py import them (cooc_sparse_cases itself does
    # `import cooc_defs`): one identity for each, whoever imports first
    if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import cooc_defs
    import cooc_sparse_cases as csc
    U, M = 700, 40
    raw, item = csc.planted(U, M, 2000, 3, seed=5, plant=False)
    rename = np.random.RandomState(6).permutation(M)
    sets = []
    for it in (np.asarray(item), rename[np.asarray(item)]):
        P = cooc._Prep(np.array(raw), np.array(it), M, torch.device("cpu"))
        eptr, eitem, emult = P.by_user()
        s = {k: _c(getattr(P, k).numpy()) for k in ("iptr", "iuser", "iitem", "imult", "uptr", "uitem", "upos")}
        s.update(eptr=_c(eptr.numpy()), eitem=_c(eitem.numpy()), emult=_c(emult.numpy()), order=_c(P.row_order().numpy()))
        t = cooc_defs.pair_table(raw, it, M)
        keep = t["count"] >= _COOC_THR
        o = np.lexsort((t["b"][keep], t["a"][keep]))
        a, b, cnt, u, p, q = (t[k][keep][o] for k in ("a", "b", "count", "u", "p", "q"))
        s["records"] = _c(np.stack([a, b, cnt, u // csc.WINDOW], axis=1), np.int32)
        up = s["uptr"][u]
        s["keys"] = _c((up + p) * P.R + (up + q), np.int64)
        s["perm"] = _c(np.argsort(s["keys"], kind="stable"), np.int64)
        s["edge_index"], s["edge_weight"] = (_c(x) for x in cooc_defs.item_similarity_graph(raw, it, M, _COOC_THR))
        m, iu, ii = (s[k].astype(np.int64) for k in ("imult", "iuser", "iitem"))
        stats = np.zeros((3, M), np.int64)
        np.add.at(stats[0], ii, m * (m - 1) // 2)
        np.add.at(stats[1], ii, m * m)
        stats[2] = 0x7f7f7f7f7f7f7f7f
        np.minimum.at(stats[2], ii[m >= 2], iu[m >= 2])
        s.update(item_stats=_c(stats.reshape(-1)), max_seen=np.array([P.max_mult], np.int32), count=np.array([len(a)], np.int64))
        s["dims"] = dict(U=P.U, M=M, R=P.R, n=len(m), max_mult=P.max_mult, max_sq=P.max_sq(), pairs=len(a))
        sets.append(s)
    da, db = sets[0]["dims"], sets[1]["dims"]
    assert da == db and da["U"] > csc.WINDOW and da["pairs"] > 50 and da["max_mult"] == 3
    assert len({int(w) for w in sets[0]["records"][:, 3]}) == 2              # first users in both windows
    return da, sets


def _cooc_pairs_out(d):
    cap = d["pairs"] + 7
    return cap, {"records": ((cap, 4), np.int32), "count": ((1,), np.int64), "h_count": ((1,), np.int64)}


@case
def _ps_cooc_planes(name):
    """item_stats / max_seen restated from the header's three sums; the operand planes have no restatement: eager expectation"""
    d, sets = _cooc_sets()
    n = int(lib().ps_cooc_planes_bytes(d["U"], d["M"], d["max_mult"]))
    assert n > 0
    return Case(name, [I("iuser"), I("iitem"), I("imult"), d["n"], d["U"], d["M"], d["max_mult"], O("planes"), n, O("item_stats"),
                       O("max_seen"), ST], tuple(_pick(s, "iuser", "iitem", "imult") for s in sets),
                {"planes": ((n,), np.uint8), "item_stats": ((3 * d["M"],), np.int64), "max_seen": ((1,), np.int32)},
                tuple(_pick(s, "item_stats", "max_seen") for s in sets))


@case
def _ps_cooc_pairs(name):
    d, sets = _cooc_sets()
    n = int(lib().ps_cooc_planes_bytes(d["U"], d["M"], d["max_mult"]))
    cap, outs = _cooc_pairs_out(d)
    ins = tuple({"planes": np.zeros(n, np.uint8) + np.uint8(i), "item_stats": s["item_stats"]} for i, s in enumerate(sets))
    return Case(name, [I("planes"), d["U"], d["M"], d["max_mult"], d["max_sq"], I("item_stats"), _COOC_THR, O("records"), cap,
                       O("count"), HO("h_count"), ST], ins, outs, tuple(_pick(s, "records", "count") for s in sets),
                unordered={"records": "count"}, host_copy={"h_count": "count"}, synchronises=True, derived={"planes": ("ps_cooc_planes", "planes")})


@case
def _ps_cooc_pairs_sparse(name):
    d, sets = _cooc_sets()
    cap, outs = _cooc_pairs_out(d)
    ins = ("iptr", "iuser", "imult", "eptr", "eitem", "emult", "order")
    return Case(name, [I("iptr"), I("iuser"), I("imult"), I("eptr"), I("eitem"), I("emult"), I("order"), d["n"], d["U"], d["M"],
                       d["max_sq"], _COOC_THR, 0, O("records"), cap, O("count"), HO("h_count"), WS, WSB, ST],
                tuple(_pick(s, *ins) for s in sets), outs, tuple(_pick(s, "records", "count") for s in sets),
                unordered={"records": "count"}, host_copy={"h_count": "count"}, synchronises=True, ws=("ps_cooc_pairs_sparse_workspace_bytes", (d["M"], 0)))


@case
def _ps_cooc_keys(name):
    d, sets = _cooc_sets()
    ins = ("records", "iptr", "iuser", "imult", "uptr", "uitem", "upos")
    return Case(name, [I("records"), d["pairs"], d["U"], d["M"], I("iptr"), I("iuser"), I("imult"), I("uptr"), I("uitem"), I("upos"),
                       d["R"], O("keys"), ST], tuple(_pick(s, *ins) for s in sets), {"keys": ((d["pairs"],), np.int64)},
                tuple(_pick(s, "keys") for s in sets))


@case
def _ps_cooc_emit(name):
    d, sets = _cooc_sets()
    n = d["pairs"]
    return Case(name, [I("records"), I("perm"), n, O("edge_index"), O("edge_weight"), ST], tuple(_pick(s, "records", "perm") for s in sets),
                {"edge_index": ((2, 2 * n), np.int64), "edge_weight": ((2 * n,), np.float32)},
                tuple(_pick(s, "edge_index", "edge_weight") for s in sets))


# further cases of an entry point that has one above: "<entry point>:<form>"
VARIANTS = {"ps_mt19937_random_sample:serial": functools.lru_cache(maxsize=None)(lambda: _mt_serial("ps_mt19937_random_sample")),
            "ps_lsh_expand:queries": functools.lru_cache(maxsize=None)(lambda: _expand_queries("ps_lsh_expand"))}
