"""What the C entries of the mesh index kernels (marching cubes dense and streamed, connected components with compaction, vertex clustering) refuse, and what
their *_scratch entries return, without a GPU: tests/golden/mesh_entry_rules.json -- recorded by tests/golden/make_mesh_entry_rules.py at the commit named in its
header, before the scratch walks and the shared refusals became one host header -- replayed against the built library.  Every cell is a call that is refused
before any device work: nothing here launches.

Equal in every cell and byte for byte: the status code, the whole ac_last_error() text, every scratch size."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_mesh_entry_rules", os.path.join(HERE, "golden", "make_mesh_entry_rules.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fixture(G):
    with open(G.FIXTURE) as f:
        doc = json.load(f)
    assert len(doc["header"]["parent_commit"]) == 40 and doc["header"]["mesh"] == [G.V, G.T, G.NC]
    assert doc["entries"] == list(G.ENTRIES) and len(doc["entries"]) == 14
    assert {e: list(r) for e, r in doc["rows"].items()} == {e: list(r) for e, r in G.ROWS.items()}      # the stored matrix is the generator's: nothing dropped on either side
    assert sorted(list(doc["rows"]) + doc["mesh_scratch"] + doc["grid_scratch"]) == sorted(G.ENTRIES)   # every entry is replayed, as a refusal table or as sizes
    return doc


def test_refusals_equal_the_parent_commit():
    from avatarcraft_amd import _lib as L
    G = _generator()
    doc = _fixture(G)
    n_cells = 0
    for entry, rows in doc["rows"].items():
        for row, then in rows.items():
            assert then[0] == G.AC_ERR_BAD_ARG and then[1].startswith(entry[3:] + ": "), (entry, row, then)
            got = G.call(L, entry, row)
            assert got == then, f"{entry} x {row}:\n  parent {then}\n  now    {got}"
            n_cells += 1
    assert n_cells == 120


def test_scratch_sizes_equal_the_parent_commit():
    from avatarcraft_amd import _lib as L
    G = _generator()
    doc = _fixture(G)
    assert (doc["mesh_scratch"], doc["grid_scratch"]) == (list(G.MESH_SCRATCH), list(G.GRID_SCRATCH))
    assert [tuple(r[:2]) for r in doc["scratch"]["shapes"]] == G.SHAPES and [tuple(r[:3]) for r in doc["scratch"]["grids"]] == G.GRIDS
    for want in ((0, 0), (1, 0), (3, 1), (1024, 1024), (1025, 1), (1, 1025), (2049, 5), (97492, 194980), (1580000, 3160000), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert want in G.SHAPES
    for want in ((2, 2, 2), (3, 2, 2), (48, 48, 48), (66, 512, 512), (512, 512, 512), (1290, 1290, 1290), (1296, 1296, 1296)):
        assert want in G.GRIDS
    assert G.record_scratch(L) == doc["scratch"]
