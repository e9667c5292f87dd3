"""An edit for the capture-once, edit, replay loop of a prepared smallpt scene,
checked on the CPU: an emitter moved and re-tinted with the light count kept
is the update a captured launch must see (nothing it holds by value changes).
The oracle alone must tell the edited scene from the base one, or a replay
that ignored the edit could pass a comparison built on it."""
import pytest

import graph_edits_check as ge
import refit_check as rc
import scenes_layouts as sl
import spt_check


@pytest.mark.parametrize("mode", [0, 1], ids=["pt", "dl"])
def test_emitter_edit_changes_the_oracles_frame(oracle, mode):
    """cloud(3000), 64 x 48 at 2 spp: emitter 3 moved by a quarter of the
    cloud's extent and scaled by (2, 0.5, 1) changes at least 16 pixels of the
    oracle's frame in both estimators (measured: 1,187 of 3,072 in path
    tracing, 1,175 in direct lighting); one sphere changes, the light count
    stays."""
    w, h = ge.FRAME
    S, n = sl.cloud(sl.N_LEAF8)
    rows = rc.raw_rows(S, n)
    new = ge.emitter_edit(rows)
    assert ((rows != new).any(axis=1).nonzero()[0] == [ge.EMITTER]).all()
    assert (new[:, 4:7] != 0).any(axis=1).sum() == (rows[:, 4:7] != 0).any(axis=1).sum() == 3
    cam = sl.cloud_camera(w, h)
    frames = [spt_check.oracle_frame(oracle, w, h, [ge.SPP], mode, (rc.from_raw(r), n), cam) for r in (rows, new)]
    differ = ge.pixels_differing(*frames)
    print("emitter edit, mode %d: %d of %d pixels differ" % (mode, differ, w * h))
    assert differ >= 16
