"""What the ten C entries of the ray renderers refuse, without a GPU: tests/golden/render_entry_rules.json -- recorded by
tests/golden/make_render_entry_rules.py at the commit named in its header, before the entries' checks became one function -- replayed against the built
library.  Every cell is a call that is refused before any device work, or a call with n_rays = 0: nothing here launches (a cell the parent accepted
at 16 rays is named in the file, not replayed).

Equal in every cell: the status code; the ac_last_error() text behind its first ": " (the prefix may have become the entry's name); the scratch numbers.
The cells listed under "amended" are the one deliberate difference (the generator's docstring): they are compared with their new answer."""
import ctypes as C
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_render_entry_rules", os.path.join(HERE, "golden", "make_render_entry_rules.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rule(status_message):
    status, msg = status_message
    return [status, msg.split(": ", 1)[1] if ": " in msg else msg]


def _fixture(G):
    with open(G.FIXTURE) as f:
        doc = json.load(f)
    assert len(doc["header"]["parent_commit"]) == 40
    assert doc["entries"] == list(G.ENTRIES) and list(doc["rows"]) == list(G.ROWS)          # the stored matrix is the generator's: nothing dropped on either side
    assert (doc["header"]["n_rays"], tuple(doc["header"]["counts"])) == (G.VALID["n_rays"], G.VALID["counts"])
    return doc


def test_rules_equal_the_parent_commit():
    from avatarcraft_amd import _lib as L
    G = _generator()
    doc = _fixture(G)
    assert doc["amended"] == G.amended()
    now = {(c["row"], c["entry"]): c["now"] for c in doc["amended"]}
    n_cells = 0
    for row, r in doc["rows"].items():
        assert sorted(list(r["n16"]) + r["launches"]) == sorted(G.ENTRIES), row              # every entry of a row is either refused or named as launching
        assert ("n0" in r) == (row in G.N0_ROWS) and all(st == G.AC_ERR_BAD_ARG for st, _ in r["n16"].values()), row
        for entry, then in r["n16"].items():
            got = G.call(L, entry, row)
            assert _rule(got) == _rule(then), f"{entry} x {row} at 16 rays:\n  parent {then}\n  now    {list(got)}"
            n_cells += 1
        for entry, then in r.get("n0", {}).items():
            want = now.pop((row, entry), then)
            if want is not then:
                assert then == [0, ""] and want[0] == G.AC_ERR_BAD_ARG, (row, entry)       # an amended cell is one the early return used to hide
            got = G.call(L, entry, row, n_rays=0)
            assert _rule(got) == _rule(want), f"{entry} x {row} at 0 rays:\n  parent {then}\n  now    {list(got)}"
            n_cells += 1
    assert not now, now                                                                      # every amended cell exists in the table
    assert n_cells == 254 + 360


def test_amended_cells_are_the_permitted_kind():
    """only: an entry of the short window, n_rays = 0, an invalid precision / skip_masked / opacity_only / near-far pairing, AC_OK before"""
    G = _generator()
    doc = _fixture(G)
    assert len(doc["amended"]) == 28
    for c in doc["amended"]:
        assert c["row"] in ("precision_7", "skip_masked_2", "opacity_only_2", "near_m_only", "far_m_only") and not G.ENTRIES[c["entry"]][0]
        assert c["parent"] == [0, ""] == doc["rows"][c["row"]]["n0"][c["entry"]]
        assert _rule(c["now"]) == _rule(doc["rows"][c["row"]]["n16"][c["entry"]])          # the rule the same call names at 16 rays


def test_warped_scratch_layout_equals_the_parent_commit():
    from avatarcraft_amd import _lib as L
    G = _generator()
    doc = _fixture(G)
    assert [(n, t) for n, t, _, _ in doc["scratch"]] == G.SCRATCH_SHAPES
    assert G.record_scratch(L) == doc["scratch"]
    assert L.lib().ac_render_rays_warped_scratch(16, 164, None) == doc["scratch"][2][2]     # offs may be NULL
    offs = (C.c_size_t * 6)()
    assert L.lib().ac_render_rays_warped_scratch(-3, -1, offs) == 0 and list(offs) == [0] * 6
