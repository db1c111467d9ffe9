"""The personalized-PageRank cases without a GPU: the plain-python restatement of the reference's push loop and the
level-scheduled pull model of tests/helpers/ppr_cases.py (the arithmetic of csrc/ppr_push.hip) both reproduce the reference's
recorded scores bit for bit, the cases tell the pull model from four near misses, and the table covers what it says."""
import ast
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ppr_cases as pc  # noqa: E402


def _scores(name, fn, **kw):
    _, _, sources, alpha, sweeps, _ = pc.case(name)
    adj, size = pc.adjacency(name), pc.size_of(name)
    return np.array([fn(adj, size, s, alpha, sweeps, **kw) for s in sources], dtype=np.float64)


@pytest.mark.parametrize("name", pc.NAMES)
def test_fixture_holds_the_case_inputs(name):
    g = pc.golden()
    ei, ew, sources, alpha, sweeps, k = pc.case(name)
    assert np.array_equal(g[f"{name}_edge_index"], ei) and np.array_equal(g[f"{name}_edge_weights"], ew)
    assert g[f"{name}_edge_weights"].dtype == np.float32 and g[f"{name}_scores"].dtype == np.float64
    assert list(g[f"{name}_sources"]) == list(sources) and float(g[f"{name}_alpha"]) == alpha
    assert int(g[f"{name}_sweeps"]) == sweeps and int(g[f"{name}_k"]) == k
    assert g[f"{name}_scores"].shape == (len(sources), pc.size_of(name))


@pytest.mark.parametrize("name", pc.NAMES)
def test_restated_push_loop_equals_the_reference(name):
    assert np.array_equal(_scores(name, pc.reference_scores), pc.golden()[f"{name}_scores"])


@pytest.mark.parametrize("name", pc.NAMES)
def test_level_scheduled_pull_model_equals_the_reference(name):
    assert np.array_equal(_scores(name, pc.pull_scores), pc.golden()[f"{name}_scores"])


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_cases_tell_the_pull_model_from_a_near_miss(variant):
    differing = [name for name in pc.NAMES
                 if not np.array_equal(_scores(name, pc.pull_scores, variant=variant), pc.golden()[f"{name}_scores"])]
    print(variant, "differs on", differing)
    assert differing


@pytest.mark.parametrize("name", pc.NAMES)
def test_restated_selection_equals_the_reference(name):
    """precompute_top_neighbors always runs alpha 0.15 / 10 sweeps: ids in the same order, weights equal as python floats"""
    g = pc.golden()
    _, _, sources, _, _, k = pc.case(name)
    adj, size = pc.adjacency(name), pc.size_of(name)
    for i, s in enumerate(sources):
        ids, w = pc.select(pc.pull_scores(adj, size, s, pc.DEFAULT_ALPHA, pc.DEFAULT_SWEEPS), k)
        n = int(g[f"{name}_top_nvalid"][i])
        assert ids == list(g[f"{name}_top_ids"][i, :n]) and w == list(g[f"{name}_top_w"][i, :n])
        assert np.all(g[f"{name}_top_ids"][i, n:] == -1)


def test_case_table_covers_what_it_says():
    g = pc.golden()
    lev = {name: pc.levels(pc.adjacency(name), pc.num_nodes(name)) for name in pc.NAMES}
    assert max(lev["bip10"]) + 1 == 2 and max(lev["chain"]) + 1 == 48
    assert sorted({pc.case(name)[4] for name in pc.NAMES}) == [1, 4, 10]
    # the random graph: self-loops, duplicate edges, sinks, an isolated node
    ei = pc.case("random")[0]
    assert pc.num_nodes("random") == 40 and ei.shape[1] == 300 and int((ei[0] == ei[1]).sum()) >= 8
    assert len({(int(a), int(b)) for a, b in ei.T}) <= 300 - 12
    adj = pc.adjacency("random")
    assert all(not adj[v] for v in (3, 11, 17, 26)) and 17 not in ei
    # the hub: in-degree 300 from both sides
    ei = pc.case("hub")[0]
    into = ei[0][ei[1] == pc.HUB]
    assert into.size == 300 and (into < pc.HUB).sum() == 150 and (into > pc.HUB).sum() == 150
    # a source beyond the graph, in three cases
    assert sum(max(pc.case(name)[2]) >= pc.num_nodes(name) for name in pc.NAMES) >= 3
    # exact ties across the k boundary, resolved to the smaller ids
    k = int(g["stars_k"])
    row = g["stars_scores"][0]
    assert len(set(row[1:9])) == 1 and row[1] > 0 and k == 4
    assert list(g["stars_top_ids"][0]) == [0, 1, 2, 3] and list(g["stars_top_ids"][1]) == [17, 9, 10, 11]
    # k beyond the number of positive scores
    assert (g["bip1_top_nvalid"] < int(g["bip1_k"])).all() and (g["stars_top_nvalid"][4] == 1)


# tests/manifest.txt guards the tests it lists against being dropped or renamed unnoticed; these are the names the
# personalized-PageRank work added, held here in the same way
PPR_TESTS = {
    "test_ppr_cases.py": ("test_fixture_holds_the_case_inputs", "test_restated_push_loop_equals_the_reference",
                          "test_level_scheduled_pull_model_equals_the_reference", "test_cases_tell_the_pull_model_from_a_near_miss",
                          "test_restated_selection_equals_the_reference", "test_case_table_covers_what_it_says",
                          "test_no_ppr_test_was_dropped"),
    "test_hip_ppr.py": ("test_scores_equal_the_reference", "test_level_lists", "test_source_counts_and_chunkings",
                        "test_state_byte_offsets_beyond_2_32", "test_row_skipping_changes_nothing",
                        "test_shares_equal_the_left_to_right_quotients", "test_top_neighbours_equal_the_reference",
                        "test_max_target_keeps_the_items", "test_ppr_matrix_dict", "test_host_and_device_methods_agree",
                        "test_pooling_and_forward_take_a_weighted_batch", "test_two_runs_are_bit_identical",
                        "test_bad_arguments_are_refused"),
}


def test_no_ppr_test_was_dropped():
    here = os.path.dirname(os.path.abspath(__file__))
    for fn, names in PPR_TESTS.items():
        tree = ast.parse(open(os.path.join(here, fn)).read(), filename=fn)
        have = {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
        assert not sorted(set(names) - have), f"{fn}: tests no longer defined: {sorted(set(names) - have)}"
        assert not sorted(have - set(names)), f"{fn}: add to PPR_TESTS: {sorted(have - set(names))}"
