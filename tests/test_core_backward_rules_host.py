"""What ac_render_core_backward and the stand-alone training operators refuse, without a GPU: tests/golden/core_backward_rules.json -- recorded by
tests/golden/make_core_backward_rules.py at the commit named in its header, before the whole-core backward checked all of its rules ahead of its first
launch -- replayed against the built library.  Every row is one call that breaks exactly one rule; equal in every row: the status code and the
ac_last_error() text behind its first ": " (the row's "rule": the generator's docstring says where that is not literally the recording).

The pointers of these calls are host dummies, so the replay does not run where a device exists: there, a rule the library got wrong would become a launch on
them.  Without a device such a launch only fails.  (On the device: tests/test_gpu_core_backward_refusals.py, on real buffers.)"""
import importlib.util
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def generator():
    spec = importlib.util.spec_from_file_location("make_core_backward_rules", os.path.join(HERE, "golden", "make_core_backward_rules.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fixture(G):
    with open(G.FIXTURE) as f:
        doc = json.load(f)
    assert len(doc["header"]["parent_commit"]) == 40
    assert list(doc["rows"]) == G.ROWS                                   # the stored rows are the generator's: nothing dropped on either side
    assert (doc["header"]["n_rays"], doc["header"]["counts"]) == (G.N, [G.T0, G.UP])
    return doc


def test_fixture_is_the_generators():
    """the rows whose rule is not the literal recording are exactly the four the parent reached behind a launch check, and they were recorded as that"""
    G = generator()
    doc = fixture(G)
    late = {"render_core_backward." + r: t for r, t in G.ROWS_BEHIND_LAUNCH_CHECK.items()}
    assert len(doc["rows"]) == 33 and len(late) == 4 and set(G.ROWS_BEHIND_LAUNCH_CHECK) <= set(G.ROWS_AFTER_LAUNCH) <= set(G.CORE_ROWS)
    for row, r in doc["rows"].items():
        assert r["rule"][0] == G.AC_ERR_BAD_ARG and r["rule"][1], row
        assert ("recorded" in r) == (row in late), row
        if row in late:
            assert r["rule"][1] == late[row] and r["recorded"][0] == G.AC_ERR_LAUNCH, row
    # a late rule that a stand-alone entry shares is stored in the words the parent was recorded with there
    assert doc["rows"]["render_core_backward.level_layout"]["rule"] == doc["rows"]["sdf_stencil_forward.level_layout"]["rule"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="host dummy pointers: replayed only where nothing can launch")
def test_rules_equal_the_parent_commit():
    from avatarcraft_amd import _lib as L
    G = generator()
    doc = fixture(G)
    for row, r in doc["rows"].items():
        got = G.call(L, row)
        assert got == r["rule"], f"{row}:\n  parent {r['rule']}\n  now    {got}"
