"""tests/helpers/abi_cases.py on the CPU: the table covers every entry point of include/pinsage_hip.h that takes a stream, only the
two documented entry points are exempt from capture, and every builder runs with its own assertions (the shape conditions that
make a case reach its workspace and every launch, two input sets that differ, two expectations that differ)."""
import os
import re

import pytest

from helpers import abi_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pinsage_hip.h")

# the entry points whose case leaves at least one output to the eager call (no bit-exact restatement of that output exists):
# a new name here is a decision, not an accident
EAGER = {
    "ps_attention_weights": ["attn"],           # softmax over expf
    "ps_gcn_layer": ["y"],                      # the row norm: the oracle gives a bound
    "ps_gcn_layer_ordered": ["y"],
    "ps_lsh_stage": ["staged"],                 # layouts the matrix cores consume, defined by the kernels that read them
    "ps_lsh_encode_planes": ["planes"],
    "ps_lsh_expand": ["planes"],
    "ps_hardest_negative": ["best"],
    "ps_cooc_planes": ["planes"],
}


def _stream_taking_functions():
    """the functions include/pinsage_hip.h declares with a ps_stream_t parameter (parsed as tests/test_abi.py parses it)"""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"^[ \t]*#.*$", "", txt, flags=re.M)
    out = set()
    for _, name, params in re.findall(r"([\w\s\*]+?)\b(ps_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", txt, flags=re.S):
        if re.search(r"\bps_stream_t\b", params):
            out.add(name)
    return out


def test_every_stream_taking_entry_point_has_a_case():
    want = _stream_taking_functions()
    assert len(want) >= 57
    assert set(ac.CASES) == want, (sorted(want - set(ac.CASES)), sorted(set(ac.CASES) - want))
    for name in ac.VARIANTS:                                      # a further form of an entry point that has a case
        assert name.partition(":")[0] in ac.CASES and ac.get(name).name == name.partition(":")[0]


def test_only_the_documented_entry_points_synchronise():
    sync = sorted(n for n in list(ac.CASES) + list(ac.VARIANTS) if ac.get(n).synchronises)
    assert sync == ["ps_cooc_pairs", "ps_cooc_pairs_sparse"]
    txt = open(HEADER).read()
    for name in sync:
        # the comment that describes the entry point: from its bullet to the next bullet of the block
        m = re.search(r"\* " + name + r"\s*:(.*?)(?=\n \* ps_[a-z_]+\s*:|\*/)", txt, flags=re.S)
        assert m, f"{name} has no description in the header"
        assert re.search(r"SYNCHRONISES|synchronises", m.group(1)), f"the header does not say that {name} synchronises"


@pytest.mark.parametrize("name", sorted(ac.CASES) + sorted(ac.VARIANTS))
def test_builder(name):
    c = ac.get(name)                                              # Case.__init__ and the builder assert the conditions
    a, b = c.inputs
    assert any(a[k].tobytes() != b[k].tobytes() for k in a)
    if c.expect[0]:
        assert any(c.expect[0][k].tobytes() != c.expect[1][k].tobytes() for k in c.expect[0])
    assert c.eager_outputs == EAGER.get(c.name, []), f"{name}: outputs without an independent oracle: {c.eager_outputs}"
    if c.ws is not None:
        assert c.workspace_bytes() > 0
    assert sum(len(v) for v in c.outputs.values()) + len(c.inout) > 0
    for k in c.unordered:
        assert c.expect[0][k].shape[0] > 0                        # unordered records: some survive
    total = sum(v.nbytes for v in a.values())
    assert total < 64 << 20, f"{name}: {total} bytes of input: not a small case"


def test_eager_list_names_entry_points():
    assert set(EAGER) <= set(ac.CASES)
