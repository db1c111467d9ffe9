"""ctypes binding of libpinsage_hip.so (C ABI: include/pinsage_hip.h).

There is NO fallback: if the shared library is missing every op raises LibraryMissing."""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("PS_HIP_LIB") or os.path.join(_HERE, "libpinsage_hip.so")   # PS_HIP_LIB: kernel experiments only
_lib = None

PS_RNG_STREAM = 0
PS_RNG_PHILOX = 1
PS_RNG_STREAM_RAW = 2
PS_RNG_STREAM_WALKS = 3
PS_WALK_HALF_BUCKETS = 0x100
PS_RELU = 1
PS_L2NORM = 2
PS_WPERM = 4
PS_LSH_STAGED = 8
PS_HN_PER_QUERY, PS_HN_EXCLUDE_DIAG = 1, 2
PS_LOSS_SHARED, PS_LOSS_PER_QUERY, PS_LOSS_BATCH_HARD = 0, 1, 2
PS_PPR_NO_SKIP = 1
PS_OK, PS_EINVAL, PS_ELAUNCH, PS_EWORKSPACE, PS_EUNSUPPORTED = 0, -1, -2, -3, -4      # status codes (include/pinsage_hip.h)


class LibraryMissing(RuntimeError):
    pass


class NativeError(RuntimeError):
    pass


# Every exported symbol of include/pinsage_hip.h as "<return> <parameters>", one letter per C type (tests/test_abi.py holds the
# table to the header): p any pointer or ps_stream_t, q int64_t, i int, z size_t, Q uint64_t, I uint32_t, f float,
# s const char *.  lib() turns each entry into restype / argtypes, so a call site passes plain Python values and a value of
# the wrong kind, or a missing argument, is a ctypes.ArgumentError instead of a truncated word on the device.
_CTYPES = {"p": C.c_void_p, "q": C.c_int64, "i": C.c_int, "z": C.c_size_t, "Q": C.c_uint64, "I": C.c_uint32, "f": C.c_float,
           "s": C.c_char_p}
PROTOTYPES = {
    "ps_abi_version": "i",
    "ps_error_string": "s i",
    "ps_csr_build_workspace_bytes": "z qq",
    "ps_csr_build": "i pppqqppppzp",
    "ps_cdf_build": "i ppqpp",
    "ps_guide_build": "i ppqppp",
    "ps_pack_edges": "i pppqpp",
    "ps_bucket_build": "i ppppqqpp",
    "ps_bucket_build_half": "i ppppqqpp",
    "ps_dest_info_build": "i ppqqpp",
    "ps_graph_stats": "i ppqqpp",
    "ps_walk_sample": "i pppqpqiiiippQIppppppppp",
    "ps_walk_sample_layers": "i pppqpqiiiippqQIpppppipppp",
    "ps_walk_paths": "i pppqpqiippQIipppp",
    "ps_walk_paths_biased": "i pppppqpqiippQIippp",
    "ps_paths_topk_max_entries": "i",
    "ps_paths_topk": "i pqiipppp",
    "ps_uniform_offsets": "i pqpqiippp",
    "ps_mt19937_chunk_log2": "i",
    "ps_mt19937_window_shift": "i",
    "ps_mt19937_raw_stream": "i piqppppipipipipzp",
    "ps_mt19937_workspace_bytes": "z qq",
    "ps_mt19937_random_sample": "i piqqppppipipipzp",
    "ps_importance_pool": "i pqippppqiqipp",
    "ps_attention_weights": "i ppqipppqipp",
    "ps_gather_max": "i pqippqipp",
    "ps_pool_weights": "i ppppqiqiipp",
    "ps_gather_bwd_segment": "i",
    "ps_gather_bwd_workspace_bytes": "z qii",
    "ps_gather_bwd": "i ppqipppqippzp",
    "ps_gather_max_arg": "i pqippqippp",
    "ps_attention_bwd_rows_workspace_bytes": "z qi",
    "ps_attention_bwd_rows": "i pqippipppppqippppzp",
    "ps_attention_bwd_cols": "i ppqipppipqppzp",
    "ps_bn_stats_workspace_bytes": "z qi",
    "ps_bn_batch_stats": "i pqipffppppppzp",
    "ps_bn_apply": "i pqipppipp",
    "ps_bn_bwd_workspace_bytes": "z qi",
    "ps_bn_bwd": "i ppqippppfippppzp",
    "ps_layer_norm": "i pqippfppppp",
    "ps_layer_norm_bwd_workspace_bytes": "z qi",
    "ps_layer_norm_bwd": "i ppqippppppppzp",
    "ps_permute_k": "i pqiipp",
    "ps_linear": "i pqipipipipiipp",
    "ps_linear_wgrad_partition": "q q",
    "ps_linear_wgrad_workspace_bytes": "z qii",
    "ps_linear_wgrad": "i pqipipppzp",
    "ps_linear_epilogue_bwd": "i ppqiipp",
    "ps_gcn_layer_workspace_bytes": "z qi",
    "ps_gcn_layer": "i pqipipipqippppiqipiippzp",
    "ps_gcn_order": "i ppiqiqppp",
    "ps_gcn_layer_ordered": "i pqipipipqippppiqipiippzppp",
    "ps_lsh_stage_bytes": "z ii",
    "ps_lsh_stage": "i piipzp",
    "ps_lsh_encode": "i pqipipip",
    "ps_lsh_encode_planes": "i pqipippp",
    "ps_hamming_topk_workspace_bytes": "z qqii",
    "ps_hamming_topk": "i pqpqiiqpppzp",
    "ps_lsh_planes_bytes": "z qi",
    "ps_lsh_expand": "i pqipp",
    "ps_hamming_topk_mfma_workspace_bytes": "z qqii",
    "ps_hamming_topk_mfma": "i pqpqiiqpppzp",
    "ps_hamming_topk_mfma_codes": "i pqpqiiqpppzp",
    "ps_topk_merge": "i ppiqippp",
    "ps_topk_merge_strided": "i pqpqiqippp",
    "ps_dot_topk_workspace_bytes": "z qqii",
    "ps_dot_topk": "i pqipqiipppzp",
    "ps_row_dot": "i pqpqippqpp",
    "ps_rank_count": "i pqiqpqpppp",
    "ps_rerank_max_candidates": "i",
    "ps_rerank_topk": "i pqiqpqpiippp",
    "ps_frontier_workspace_bytes": "z qqqi",
    "ps_frontier_build": "i pqppqiqppppzp",
    "ps_l2_topk_workspace_bytes": "z qqii",
    "ps_l2_topk": "i pqipqippipppzp",
    "ps_ivf_topk_workspace_bytes": "z qqiiiiq",
    "ps_ivf_topk": "i pqipiqppqpiipppzp",
    "ps_spmm_csr": "i ppppqiqqpp",
    "ps_spmm_exact_slice": "i",
    "ps_spmm_csr_exact_workspace_bytes": "z qi",
    "ps_spmm_csr_exact": "i ppppqiqqppzp",
    "ps_sddmm_csr": "i pppqpqiqpp",
    "ps_cooc_planes_bytes": "z qqi",
    "ps_cooc_planes": "i pppqqqipzppp",
    "ps_cooc_pairs": "i pqqiqpqpqppp",
    "ps_cooc_pairs_sparse_workspace_bytes": "z qi",
    "ps_cooc_pairs_sparse": "i pppppppqqqqqipqpppzp",
    "ps_cooc_keys": "i pqqqppppppqpp",
    "ps_cooc_emit": "i ppqppp",
    "ps_hardest_negative": "i pqipqipppp",
    "ps_margin_loss": "i ppqipfppppp",
    "ps_margin_loss_bwd": "i pppqqiippppppp",
    "ps_ppr_shares": "i ppqpp",
    "ps_ppr_push_workspace_bytes": "z qq",
    "ps_ppr_push": "i pppqqppipqQiippzp",
    "ps_ppr_topk": "i pqqqqippppp",
    "ps_rank_window_max": "i",
    "ps_rank_window": "i pqqqqpqqpipppp",
}
SYMBOLS = list(PROTOTYPES)


def have_lib() -> bool:
    return os.path.exists(SO_PATH)


def lib():
    global _lib
    if _lib is None:
        if not have_lib():
            raise LibraryMissing(
                f"{SO_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the PinSage hot path.")
        L = C.CDLL(SO_PATH)
        for name, code in PROTOTYPES.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise NativeError(f"{SO_PATH} does not export {name} (include/pinsage_hip.h): rebuild it") from None
            ret, _, params = code.partition(" ")
            fn.restype, fn.argtypes = _CTYPES[ret], [_CTYPES[c] for c in params]
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        raise NativeError(f"{what}: {lib().ps_error_string(rc).decode()} (code {rc})")


class KernelTimer:
    """Optional per-launch HIP-event timing (events are recorded on the stream the kernels are
    launched on, torch's current stream; nothing synchronises until `summary`)."""

    def __init__(self):
        self.events = []

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.events:
            d = out.setdefault(name, {"launches": 0, "ms": 0.0})
            d["launches"] += 1
            d["ms"] += a.elapsed_time(b)
        for d in out.values():
            d["avg_ms"] = d["ms"] / d["launches"]
        return out


_timer = None


def set_timer(t):
    global _timer
    _timer = t


# entry points that the per-launch timer books under another call's name: the encode that also writes the planes is an encode
_TIMER_NAMES = {"ps_lsh_encode_planes": "ps_lsh_encode"}


def call(name, *args, unsupported_ok=False):
    """Invoke one C-ABI entry point and raise on a non-zero status.  Returns the status, which is therefore always PS_OK --
    unless unsupported_ok is set: then PS_EUNSUPPORTED is returned, not raised, for a caller that has another way."""
    fn = getattr(lib(), name)
    if _timer is None:
        rc = fn(*args)
    else:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(*args)
        b.record()
        _timer.events.append((_TIMER_NAMES.get(name, name), a, b))
    if unsupported_ok and rc == PS_EUNSUPPORTED:
        return rc
    check(rc, name)
    return rc


def ptr(t, contiguous=True):
    """Device pointer of a contiguous CUDA tensor (None -> NULL); contiguous=False takes a strided view as it is (a weight
    matrix passed with its leading dimension)."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise NativeError("libpinsage_hip takes device (HBM) pointers; got a CPU tensor")
    if contiguous and not t.is_contiguous():
        raise NativeError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def workspace(bytes_fn, device, *dims):
    """(uint8 scratch tensor on `device`, its size in bytes) as the library's `bytes_fn` sizes it for `dims`; (None, 0) when it
    answers 0 -- whether that means "nothing needed" or "shape not served" is the caller's to know."""
    nbytes = getattr(lib(), bytes_fn)(*dims)
    return (torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None), nbytes


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_get_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """torch's current HIP stream of the current device as a C pointer.  (torch.cuda.current_stream() builds a python Stream object
    through three layers of device-index helpers: 9 us a call, 14 calls per step -- a quarter of a sharded step's host time.)"""
    if _raw_stream is not None and _get_device is not None:
        return C.c_void_p(_raw_stream(_get_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu():
    if not torch.cuda.is_available():
        raise NativeError("the PinSage hot path needs an MI355X (torch.cuda is not available); "
                          "there is no CPU fallback")
    lib()
    return torch.device("cuda", torch.cuda.current_device())


# the scalar types of the table by name, for callers of exports outside it (ps_debug_*: tools/) and for tests
i64 = C.c_int64
i32 = C.c_int
u64 = C.c_uint64
u32 = C.c_uint32
