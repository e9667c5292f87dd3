"""Inputs of the capture-once, edit, replay checks of a prepared smallpt scene
("Captured graphs across scene edits"): the emitter edit
that keeps the light count, and the frame comparison its CPU check uses
(tests/test_graph_edits_inputs.py).

TEST INFRASTRUCTURE ONLY (imported like refit_check and spt_check)."""
import numpy as np

SPP = 2
FRAME = (64, 48)

# ---- the emitter edit (cloud(3000): sphere 0 the ground, 1..3 the emitters) ----
EMITTER = 3
EMITTER_SCALE = (2.0, 0.5, 1.0)


def emitter_edit(rows):
    """cloud3000's third emitter moved along x by a quarter of the cloud's
    extent, its emission scaled per channel by EMITTER_SCALE: the light count
    stays, no material is touched."""
    out = rows.copy()
    extent = float(np.ptp(rows[4:, 1:4], axis=0).max())
    out[EMITTER, 1] += np.float32(extent / 4)
    out[EMITTER, 4:7] *= np.array(EMITTER_SCALE, np.float32)
    return out


def pixels_differing(a, b):
    """Pixels whose colour bits differ between two (colors, ...) frames."""
    return int((a[0].view(np.uint32).reshape(-1, 3) != b[0].view(np.uint32).reshape(-1, 3)).any(axis=1).sum())
