"""CPU-only: every exported symbol of include/loamx.h whose name contains "_dev" is enqueued by a row of the stream table of
tests/test_gpu_streams.py, or stands in EXCLUDED with its reason. A new device entry point cannot arrive without a stream case,
and a row cannot leave the table without this test noticing."""
import os
import re

import test_gpu_streams as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXCLUDED = {
    "loamx_dev_alloc": "an allocator: it enqueues nothing",
    "loamx_dev_free": "an allocator: it synchronises by design and enqueues nothing",
    "loamx_synth_scan_pairs_dev": "a generator of inputs for tests and the benchmark",
    "loamx_gather_results_dev": "needs an RCCL communicator; covered at one rank in tests/test_gpu_multi.py",
}

# the rows of the table by name: one deleted from tests/test_gpu_streams.py, even one whose symbols another row covers, is missed here
ROWS = (
    "extract", "extract_f32", "feature_batch", "scan_pairs_dev", "scan_pairs_dev_f32", "scan_pairs_info_dev", "scan_pairs_info_dev_f32",
    "scan_sequence_dev", "scan_sequence_dev_f32", "scan_sequence_info_dev", "scan_sequence_info_dev_f32", "compose_trajectory_3",
    "compose_trajectory_65", "deskew", "deskew_f32", "organize", "organize_f32", "voxel_filter", "place_descriptors", "place_descriptors_f32",
    "place_search", "place_add_then_search", "place_add_growth_then_search", "pose_graph_edges", "pose_graph_optimize",
    "pose_graph_optimize_bad_edge", "pose_graph_edges_then_optimize", "cloud_map_add_emit", "cloud_map_add_f32_emit", "cloud_map_add_clear_add_emit",
    "occupancy_add_query_box_slice", "occupancy_add_f32_query_box_slice", "occupancy_add_clear_add_query_box_slice", "segment", "segment_f32",
    "visibility_votes_then_filter", "visibility_votes_accumulate_then_filter", "visibility_votes_f32_then_filter",
    "visibility_votes_f32_accumulate_then_filter",
)


def dev_symbols():
    header = open(os.path.join(ROOT, "include", "loamx.h")).read()
    declared = sorted(set(re.findall(r"\b(loamx_[a-z0-9_]+)\s*\(", header)))
    assert len(declared) > 100, "no declarations parsed"
    # "_dev" as a word of the name: loamx_copy_to_device (a synchronous copy helper) has none
    return [s for s in declared if re.search(r"_dev(_|$)", s)]


def test_every_dev_symbol_has_a_stream_row_or_a_reason():
    symbols = dev_symbols()
    assert len(symbols) >= 40
    in_table = {s for case in T.CASES for s in case.symbols}
    assert in_table, "the stream table is empty"
    for s in symbols:
        assert (s in in_table) != (s in EXCLUDED), f"{s}: a '_dev' entry point is a row of the stream table or excluded with a reason, one of the two"
    assert in_table <= set(symbols) | {"loamx_cloud_map_clear", "loamx_occupancy_clear"}, sorted(in_table - set(symbols))
    assert set(EXCLUDED) <= set(symbols), "an exclusion names no symbol of the header"
    assert len(EXCLUDED) == 4  # (the cap: the four named above and no more)
    assert {"loamx_cloud_map_clear", "loamx_occupancy_clear"} <= in_table  # (asynchronous on the stream as well, without "_dev" in the name)


def test_the_table_is_what_the_gpu_run_parametrises():
    marks = [m for m in T.test_gated_call.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[1] is T.CASES
    names = [c.name for c in T.CASES]
    assert len(set(names)) == len(names)
    assert tuple(names) == ROWS, (sorted(set(ROWS) - set(names)), sorted(set(names) - set(ROWS)))
    for case in T.CASES:
        assert case.klass in ("a", "b") and case.symbols and case.outputs, case.name
    # class b is what the header says waits on the host: the registration family and the database growth, nothing else
    assert {c.name for c in T.CASES if c.klass == "b"} == {c.name for c in T.REGISTRATION_ROWS} | {"place_add_growth_then_search"}
    assert all(r in T.CASES for r in T.REGISTRATION_ROWS) and len(T.REGISTRATION_ROWS) == 9
    # the pairs on objects with state, and the chain's twelve steps
    for pair in (("loamx_cloud_map_add_clouds_dev", "loamx_cloud_map_emit_dev"), ("loamx_occupancy_add_clouds_dev", "loamx_occupancy_query_dev"),
                 ("loamx_place_db_add_dev", "loamx_place_search_dev"), ("loamx_visibility_votes_dev", "loamx_visibility_filter_dev"),
                 ("loamx_pose_graph_edges_from_results_dev", "loamx_pose_graph_optimize_dev")):
        assert any(set(pair) <= set(c.symbols) for c in T.CASES), pair
    assert len(T.Chain.SYMBOLS) == 12 and all("loamx_" + s in dev_symbols() for s in T.Chain.SYMBOLS)
