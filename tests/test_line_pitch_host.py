"""The pitch of the state between the X and the Y sweep of a pair (blocking.line_pitch = armon_hip_sweep_pair_pitch): the
block's own pitch rounded up to a whole number of 128-B lines, ghost offsets kept."""
import pytest


@pytest.mark.parametrize("nx,g,itemsize,want", [
    (16384, 4, 8, 16400),         # the headline shape: 16392 doubles -> 1025 lines
    (16376, 4, 8, 16384),         # whole lines already: unchanged
    (64, 4, 8, 80), (56, 4, 8, 64), (61, 4, 8, 80), (64, 5, 8, 80), (300, 4, 8, 320), (1, 2, 8, 16),
    (16384, 4, 4, 16416), (56, 4, 4, 64),
])
def test_line_pitch_rule(nx, g, itemsize, want):
    from armon_amd.blocking import BlockSize, line_pitch
    P = line_pitch(nx, g, itemsize)
    per_line = 128 // itemsize
    assert P == want
    assert P % per_line == 0 and nx + 2 * g <= P < nx + 2 * g + per_line
    bs = BlockSize((nx + 2 * g, 40 + 2 * g), g)
    assert bs.line_pitch(itemsize) == P and bs.line_cells(itemsize) == P * (40 + 2 * g) >= bs.n_cells
    # the last real cell of the last row lies inside an array of line_cells elements, at the ghost offsets of the layout
    assert (40 - 1 + g) * P + (nx - 1) + g < bs.line_cells(itemsize)


def test_the_library_states_the_same_rule():
    import armon_amd
    from armon_amd.blocking import line_pitch
    L = armon_amd.lib()
    for nx in (1, 7, 56, 61, 64, 300, 16376, 16384, 16385):
        for g in (2, 4, 5):
            assert L.armon_hip_sweep_pair_pitch(nx, g) == line_pitch(nx, g, 8)
